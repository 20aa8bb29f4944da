// kd_encode.hip -- gfx950 kernels for VolumeKdtree::build (reference
// volume_renderer/VolumeKdTree_recover.cpp:17-140, "R.cpp").  Batched over the
// bricks of a brickset: blockIdx.y (or blockIdx.x for per-brick control kernels)
// selects the brick.  No MFMA: this is byte/integer work bound by HBM and, for the
// running-mean estimator, by a true sequential dependency.
//
// Stages
//   pyramid   R.cpp:143-201  bottom-up min/max -> midrange heap `temp`
//   compress  R.cpp:206-384  per level: serial running-mean start distance,
//                            <= maxEpochs clamped gradient-descent epochs; the GD
//                            control flow runs on the device (k_control) so the
//                            whole build is one launch sequence without host syncs
//   prune     R.cpp:596-629  bottom-up, level synchronous (race free, == serial)
//   convert   R.cpp:631-724  preorder emission by a prefix sum over leaf ranks:
//                            leaf rank r owns the tokens of the live internal
//                            nodes whose first leaf is r, then its own leaf token
//                            and grown chain
#include "brickset.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace vr {

#define EMIT_RANKS_PER_BLOCK 256     // (FILL_NODES_PER_BLOCK, FILL_ITERS: host_plan.h)

// ---------------------------------------------------------------- pyramid ----
// One block reduces 2^L inputs (L <= 10) at depth dLeaf and writes the midranges of
// depths dLeaf-1 .. dLeaf-L; the block root's (min,max) goes to outMin/outMax so the
// next round can continue upwards.  FROM_VOXELS gathers voxels in Morton order and
// also writes the leaf level.
template <bool FROM_VOXELS>
__global__ void __launch_bounds__(256)
k_pyramid(Geom g, int dLeaf, int L, const uint8_t *__restrict__ vox, const uint8_t *__restrict__ inMin,
          const uint8_t *__restrict__ inMax, int64_t inStride, uint8_t *__restrict__ temp, int64_t heapStride,
          uint8_t *__restrict__ tempRange, uint8_t *__restrict__ outMin, uint8_t *__restrict__ outMax,
          int64_t outStride, const uint32_t *__restrict__ srcIdx)
{
    __shared__ uint8_t smn[2][1024], smx[2][1024];
    const int brick = blockIdx.y;
    const uint32_t n = 1u << L;
    const uint32_t base = blockIdx.x << L;
    uint8_t *T = temp + (int64_t)brick * heapStride;
    uint8_t *TR = tempRange ? tempRange + (int64_t)brick * heapStride : nullptr;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        uint32_t r = base + i;
        uint8_t mn, mx;
        if (FROM_VOXELS) {
            int64_t vi;
            if (srcIdx) vi = srcIdx[r];            // general extents: the min corner of the leaf's box (BrickSet::srcIdx)
            else {
                int x, y, z;
                rank_to_xyz(g, r, x, y, z);
                vi = x + (int64_t)g.X * (y + (int64_t)g.Y * z);
            }
            uint8_t v = vox[(int64_t)brick * g.voxels + vi];
            mn = mx = v;
            T[((int64_t)1 << dLeaf) + r] = v;       // leaf: (v+v)/2 = v  (R.cpp:194-198)
            if (TR) TR[((int64_t)1 << dLeaf) + r] = 0; // half range of a single voxel (M.cpp:235)
        } else {
            mn = inMin[(int64_t)brick * inStride + r];
            mx = inMax[(int64_t)brick * inStride + r];
        }
        smn[0][i] = mn;
        smx[0][i] = mx;
    }
    __syncthreads();
    for (int l = 1; l <= L; ++l) {
        const uint32_t m = n >> l;
        const int src = (l - 1) & 1, dst = l & 1;
        const int da = dLeaf - l;
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
            uint8_t a = smn[src][2 * i], b = smn[src][2 * i + 1];
            uint8_t c = smx[src][2 * i], d = smx[src][2 * i + 1];
            uint8_t mn = a < b ? a : b, mx = c > d ? c : d;
            smn[dst][i] = mn;
            smx[dst][i] = mx;
            int64_t idx = ((int64_t)1 << da) + (base >> l) + i;
            T[idx] = (uint8_t)(((int)mx + (int)mn) >> 1);      // (byte)((max+min)/2.0) R.cpp:198
            if (TR) TR[idx] = (uint8_t)(((int)mx - (int)mn) >> 1); // M.cpp:235
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        outMin[(int64_t)brick * outStride + blockIdx.x] = smn[L & 1][0];
        outMax[(int64_t)brick * outStride + blockIdx.x] = smx[L & 1][0];
    }
}

// level arrays are written by one whole-volume pass and read by the next: nothing of them survives in a cache until
// then, so the large stores stream past it
__device__ __forceinline__ void st16(void *p, uint4 v)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_nontemporal_store(t, (u32x4 *)p);
}
__device__ __forceinline__ void st8(void *p, uint2 v)
{
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 t; t.x = v.x; t.y = v.y;
    __builtin_nontemporal_store(t, (u32x2 *)p);
}
__device__ __forceinline__ void st4(void *p, uint32_t v)
{
    __builtin_nontemporal_store(v, (uint32_t *)p);
}

__device__ __forceinline__ uint4 ld16(const void *p)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 t = __builtin_nontemporal_load((const u32x4 *)p);
    return make_uint4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ uint2 ld8(const void *p)
{
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 t = __builtin_nontemporal_load((const u32x2 *)p);
    return make_uint2(t.x, t.y);
}

// Bottom 12 levels in one block: the 4096 leaves under one depth-(D-12) node form a
// 2^ax x 2^ay x 2^az box (ax+ay+az = 12).  With ax >= 4 every thread fetches one aligned
// 16-byte x-run of voxels (coalesced), scatters it to Morton order in LDS, and the block
// reduces min/max twelve times there; leaves and the dense levels leave as 16/8/4-byte
// stores.  Replaces the per-voxel gather of k_pyramid<true>.
struct Pyr12Geom {
    int ax, ay, az; uint16_t sx[16];   // sx[i]: Morton rank bits of x = i (low 4 x bits)
    // XCD-aware block order (swz != 0): the eight 16-voxel-wide boxes that share every 128-byte line of an
    // x-run go to the same XCD (workgroup id mod 8) back to back, so that XCD's L2 fetches each line once
    int swz, nbx, nby, lnbx, lnby;     // lnbx, lnby = log2
    const uint32_t *spread;            // BrickSet::spread
};

// (min,max) of sibling pairs held in packed 16-bit lanes: A = (a0,a1), B = (b0,b1) -> (f(a0,a1), f(b0,b1))
__device__ __forceinline__ vr_s16x2 pk_pair_min(uint32_t A, uint32_t B)
{
    return __builtin_elementwise_min(pk_s(__builtin_amdgcn_perm(B, A, 0x05040100u)), pk_s(__builtin_amdgcn_perm(B, A, 0x07060302u)));
}
__device__ __forceinline__ vr_s16x2 pk_pair_max(uint32_t A, uint32_t B)
{
    return __builtin_elementwise_max(pk_s(__builtin_amdgcn_perm(B, A, 0x05040100u)), pk_s(__builtin_amdgcn_perm(B, A, 0x07060302u)));
}
__device__ __forceinline__ uint32_t pk_mid(vr_s16x2 mn, vr_s16x2 mx) { return pk_u((mn + mx) >> 1); }   // R.cpp:198
__device__ __forceinline__ uint32_t pk_half_range(vr_s16x2 mn, vr_s16x2 mx) { return pk_u((mx - mn) >> 1); } // M.cpp:235

// the parts k_pyramid12 and k_pyramid12_lines share (defined behind k_pyramid12)
__device__ __forceinline__ void pyr12_reduce_box(const uint8_t *leaf, int D, uint32_t base, int t, uint8_t *__restrict__ T,
                                                 uint8_t *__restrict__ TR, uint32_t *mm);
__device__ __forceinline__ void pyr12_box_root(const uint32_t *mm, int D, uint32_t base, int brick, uint8_t *__restrict__ T,
                                               uint8_t *__restrict__ TR, uint8_t *__restrict__ outMin, uint8_t *__restrict__ outMax,
                                               int64_t outStride, uint8_t *__restrict__ blockFlag, uint8_t *__restrict__ blockFlagR);

// What a constant box (every voxel c0 & 0xFF; c0 = that byte x 4) writes, in 128 slots of at most 16 bytes: levels
// D-2 .. D-12 of both heaps, the root's (min, max) and flag 1.  Levels D-1 and D stay unwritten (k_pyramid12 below).
__device__ __forceinline__ void pyr12_const_slot(int s, uint32_t c0, int D, uint32_t base, int brick, uint8_t *__restrict__ T,
                                                 uint8_t *__restrict__ TR, uint8_t *__restrict__ outMin, uint8_t *__restrict__ outMax,
                                                 int64_t outStride, uint8_t *__restrict__ blockFlag, uint8_t *__restrict__ blockFlagR)
{
    const uint4 cv = make_uint4(c0, c0, c0, c0), zv = make_uint4(0, 0, 0, 0);
    if (s < 127) {
        // 16 bytes per slot: slots 0 .. 63 level D-2, 64 .. 95 D-3, 96 .. 111 D-4, .. , 126 D-8
        const int m = s < 64 ? 0 : 5 - (31 - __clz(127 - s));             // slots 64 ..: level D-3-m
        const int k = s < 64 ? 2 : 3 + m, within = s < 64 ? s : (s - 64) - (64 - (64 >> m));
        const int64_t o = ((int64_t)1 << (D - k)) + (base >> k) + within * 16;
        st16(T + o, cv);
        if (TR) *(uint4 *)(TR + o) = zv;
    } else if (s == 127) {                      // levels D-9 .. D-12 (8, 4, 2, 1 bytes), the block's root
        const int64_t o9 = ((int64_t)1 << (D - 9)) + (base >> 9), o10 = ((int64_t)1 << (D - 10)) + (base >> 10);
        const int64_t o11 = ((int64_t)1 << (D - 11)) + (base >> 11), o12 = ((int64_t)1 << (D - 12)) + (base >> 12);
        *(uint2 *)(T + o9) = make_uint2(c0, c0);
        *(uint32_t *)(T + o10) = c0;
        *(uint16_t *)(T + o11) = (uint16_t)c0;
        T[o12] = (uint8_t)c0;
        if (TR) {
            *(uint2 *)(TR + o9) = make_uint2(0, 0);
            *(uint32_t *)(TR + o10) = 0;
            *(uint16_t *)(TR + o11) = 0;
            TR[o12] = 0;
        }
        outMin[(int64_t)brick * outStride + (base >> 12)] = (uint8_t)c0;
        outMax[(int64_t)brick * outStride + (base >> 12)] = (uint8_t)c0;
        blockFlag[(int64_t)brick * ((int64_t)1 << (D - 12)) + (base >> 12)] = 1u;
        if (blockFlagR) blockFlagR[(int64_t)brick * ((int64_t)1 << (D - 12)) + (base >> 12)] = 1u;
    }
}

__global__ void __launch_bounds__(256)
k_pyramid12(Geom g, Pyr12Geom pg, const uint8_t *__restrict__ vox, uint8_t *__restrict__ temp, int64_t heapStride,
            uint8_t *__restrict__ tempRange, uint8_t *__restrict__ outMin, uint8_t *__restrict__ outMax,
            int64_t outStride, uint8_t *__restrict__ blockFlag, uint8_t *__restrict__ blockFlagR)
{
    __shared__ __attribute__((aligned(16))) uint8_t leaf[4096];
    __shared__ uint32_t waveMM[4];
    const int brick = blockIdx.y, D = g.D;
    // which 2^ax x 2^ay x 2^az box: enumerated by box coordinates (x fastest), not by Morton index
    // (nbx, nby are powers of two -- the extents are -- so the box coordinates come from shifts and masks: the three
    // 32-bit divisions they replaced were ~200 scalar instructions in front of every wave's first load)
    uint32_t bid = blockIdx.x;
    if (pg.swz) {
        const uint32_t slot = bid >> 3;
        const uint32_t grp = (slot >> 3) * 8u + (bid & 7u), m = slot & 7u;       // group -> XCD grp % 8, members in a row
        const int lgx = pg.lnbx - 3;                                              // log2(nbx / 8)
        bid = ((grp >> lgx) << pg.lnbx) + ((grp & ((1u << lgx) - 1u)) << 3) + m;
    }
    const int bx = (int)((bid & ((1u << pg.lnbx) - 1u)) << pg.ax), by = (int)(((bid >> pg.lnbx) & ((1u << pg.lnby) - 1u)) << pg.ay),
              bz = (int)((bid >> (pg.lnbx + pg.lnby)) << pg.az);
    const uint32_t *sp = pg.spread;
    const uint32_t base = sp[bx] | sp[g.X + by] | sp[g.X + g.Y + bz];           // Morton rank of the box origin
    uint8_t *T = temp + (int64_t)brick * heapStride;
    uint8_t *TR = tempRange ? tempRange + (int64_t)brick * heapStride : nullptr;
    const int t = threadIdx.x, lane = t & 63;
    const int nxs = 1 << (pg.ax - 4);
    const int xs = t & (nxs - 1), y = (t >> (pg.ax - 4)) & ((1 << pg.ay) - 1), z = t >> (pg.ax - 4 + pg.ay);
    // Morton rank of (xs*16, y, z) inside the box (the 12 deepest split levels)
    const uint32_t r0 = sp[xs * 16] | sp[g.X + y] | sp[g.X + g.Y + z];
    const uint4 v4 = *(const uint4 *)(vox + (int64_t)brick * g.voxels + (bx + xs * 16) +
                                      (int64_t)g.X * ((by + y) + (int64_t)g.Y * (bz + z)));
    const uint32_t vw[4] = {v4.x, v4.y, v4.z, v4.w};
    // SkipBlocks builds: a box whose 4096 voxels are one value v leaves here.  Every level array of it holds v (half
    // ranges 0); levels D-2 .. D-12 go out as wide stores of the broadcast byte, levels D-1 and D are NOT written: the
    // level loop never loads them for a block it skips, and k_fill_const_leaves writes them for the others before
    // their first reader.  One barrier more than the path below, in front of the LDS transposition.
    if (blockFlag) {
        const uint32_t v0 = __builtin_amdgcn_perm(0, v4.x, 0u);                    // byte 0 x 4
        const bool mine = ((v4.x ^ v0) | (v4.y ^ v0) | (v4.z ^ v0) | (v4.w ^ v0)) == 0u;
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)v0);
        const bool waveConst = __ballot(!mine || v0 != first) == 0ull;
        if (lane == 0) waveMM[t >> 6] = waveConst ? first : 0x100u;                // (0x100: no byte x 4 looks like it)
        __syncthreads();
        const uint32_t c0 = waveMM[0];
        if (c0 != 0x100u && waveMM[1] == c0 && waveMM[2] == c0 && waveMM[3] == c0) {
            if (t < 128) pyr12_const_slot(t, c0, D, base, brick, T, TR, outMin, outMax, outStride, blockFlag, blockFlagR);
            return;
        }
        // (waveMM is written again further down, behind the barrier that follows)
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) leaf[r0 | pg.sx[i]] = (uint8_t)(vw[i >> 2] >> ((i & 3) * 8));
    __syncthreads();
    pyr12_reduce_box(leaf, D, base, t, T, TR, waveMM);
    __syncthreads();
    if (t == 0) pyr12_box_root(waveMM, D, base, brick, T, TR, outMin, outMax, outStride, blockFlag, blockFlagR);
}

// Levels D .. D-10 of one box from its Morton-ordered image `leaf` (4096 bytes of LDS, complete: the caller's barrier),
// by the 256 threads of the workgroup; mm[wave] receives the wave's packed (min, 255 - max) for pyr12_box_root.
__device__ __forceinline__ void pyr12_reduce_box(const uint8_t *leaf, int D, uint32_t base, int t, uint8_t *__restrict__ T,
                                                 uint8_t *__restrict__ TR, uint32_t *mm)
{
    const int lane = t & 63;
    // 16 Morton-consecutive leaves per thread: they and the four levels above them never leave registers
    const uint4 lv = *(const uint4 *)(&leaf[t * 16]);
    st16(T + ((int64_t)1 << D) + base + t * 16, lv);                                // leaf: (v+v)/2 = v
    if (TR) *(uint4 *)(TR + ((int64_t)1 << D) + base + t * 16) = make_uint4(0, 0, 0, 0);
    const uint32_t w[4] = {lv.x, lv.y, lv.z, lv.w};
    vr_s16x2 mn1[4], mx1[4];
    uint32_t md[4], hr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                       // level D-1: lanes = nodes 2q, 2q+1
        const vr_s16x2 lo = pk_s(w[q] & 0x00FF00FFu), hi = pk_s((w[q] >> 8) & 0x00FF00FFu);
        mn1[q] = __builtin_elementwise_min(lo, hi);
        mx1[q] = __builtin_elementwise_max(lo, hi);
        md[q] = pk_mid(mn1[q], mx1[q]);
        hr[q] = pk_half_range(mn1[q], mx1[q]);
    }
    {
        const int64_t o = ((int64_t)1 << (D - 1)) + (base >> 1) + t * 8;
        st8(T + o, make_uint2(__builtin_amdgcn_perm(md[1], md[0], 0x06040200u), __builtin_amdgcn_perm(md[3], md[2], 0x06040200u)));
        if (TR) *(uint2 *)(TR + o) = make_uint2(__builtin_amdgcn_perm(hr[1], hr[0], 0x06040200u), __builtin_amdgcn_perm(hr[3], hr[2], 0x06040200u));
    }
    vr_s16x2 mn2[2], mx2[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {                       // level D-2
        mn2[q] = pk_pair_min(pk_u(mn1[2 * q]), pk_u(mn1[2 * q + 1]));
        mx2[q] = pk_pair_max(pk_u(mx1[2 * q]), pk_u(mx1[2 * q + 1]));
    }
    {
        const int64_t o = ((int64_t)1 << (D - 2)) + (base >> 2) + t * 4;
        st4(T + o, __builtin_amdgcn_perm(pk_mid(mn2[1], mx2[1]), pk_mid(mn2[0], mx2[0]), 0x06040200u));
        if (TR) *(uint32_t *)(TR + o) = __builtin_amdgcn_perm(pk_half_range(mn2[1], mx2[1]), pk_half_range(mn2[0], mx2[0]), 0x06040200u);
    }
    const vr_s16x2 mn3 = pk_pair_min(pk_u(mn2[0]), pk_u(mn2[1])), mx3 = pk_pair_max(pk_u(mx2[0]), pk_u(mx2[1]));   // level D-3
    {
        const int64_t o = ((int64_t)1 << (D - 3)) + (base >> 3) + t * 2;
        const uint32_t m3 = pk_mid(mn3, mx3), h3 = pk_half_range(mn3, mx3);
        *(uint16_t *)(T + o) = (uint16_t)((m3 & 0xFFu) | ((m3 >> 8) & 0xFF00u));
        if (TR) *(uint16_t *)(TR + o) = (uint16_t)((h3 & 0xFFu) | ((h3 >> 8) & 0xFF00u));
    }
    int mn = min((int)mn3.x, (int)mn3.y), mx = max((int)mx3.x, (int)mx3.y);        // level D-4: one node per thread
    {
        const int64_t o = ((int64_t)1 << (D - 4)) + (base >> 4) + t;
        T[o] = (uint8_t)((mn + mx) >> 1);
        if (TR) TR[o] = (uint8_t)((mx - mn) >> 1);
    }
    // levels D-5 .. D-10 inside the wave: (min, 255 - max) packed so that one packed min reduces both
    uint32_t p = (uint32_t)mn | ((uint32_t)(255 - mx) << 16);
#pragma unroll
    for (int k = 1; k <= 6; ++k) {
        uint32_t q;
        if (k == 1) q = dpp_u32<0x101, 0xf>(p, p);          // row_shl:1 (lane i <- lane i+1)
        else if (k == 2) q = dpp_u32<0x102, 0xf>(p, p);
        else if (k == 3) q = dpp_u32<0x104, 0xf>(p, p);
        else if (k == 4) q = dpp_u32<0x108, 0xf>(p, p);
        else q = (uint32_t)__shfl_down((int)p, 1 << (k - 1));
        p = pk_u(__builtin_elementwise_min(pk_s(p), pk_s(q)));
        if ((lane & ((1 << k) - 1)) == 0) {
            const int a = (int)(p & 0xFFFFu), b = 255 - (int)(p >> 16);
            const int64_t o = ((int64_t)1 << (D - 4 - k)) + (base >> (4 + k)) + (t >> k);
            T[o] = (uint8_t)((a + b) >> 1);
            if (TR) TR[o] = (uint8_t)((b - a) >> 1);
        }
    }
    if (lane == 0) mm[t >> 6] = p;
}

// Levels D-11 (two nodes) and D-12 (the box's root) from the four waves' mm[] of pyr12_reduce_box, behind a barrier: one thread
__device__ __forceinline__ void pyr12_box_root(const uint32_t *mm, int D, uint32_t base, int brick, uint8_t *__restrict__ T,
                                               uint8_t *__restrict__ TR, uint8_t *__restrict__ outMin, uint8_t *__restrict__ outMax,
                                               int64_t outStride, uint8_t *__restrict__ blockFlag, uint8_t *__restrict__ blockFlagR)
{
    {
        int a[2], b[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t u = pk_u(__builtin_elementwise_min(pk_s(mm[2 * h]), pk_s(mm[2 * h + 1])));
            a[h] = (int)(u & 0xFFFFu); b[h] = 255 - (int)(u >> 16);
            const int64_t o = ((int64_t)1 << (D - 11)) + (base >> 11) + h;
            T[o] = (uint8_t)((a[h] + b[h]) >> 1);
            if (TR) TR[o] = (uint8_t)((b[h] - a[h]) >> 1);
        }
        const int ra = min(a[0], a[1]), rbm = max(b[0], b[1]);
        const int64_t o = ((int64_t)1 << (D - 12)) + (base >> 12);
        T[o] = (uint8_t)((ra + rbm) >> 1);
        if (TR) TR[o] = (uint8_t)((rbm - ra) >> 1);
        outMin[(int64_t)brick * outStride + (base >> 12)] = (uint8_t)ra;
        outMax[(int64_t)brick * outStride + (base >> 12)] = (uint8_t)rbm;
        // SkipBlocks: bit 0 = every voxel of the block has one value (the skip bit is set, or not, by the level loop)
        if (blockFlag) blockFlag[(int64_t)brick * ((int64_t)1 << (D - 12)) + (base >> 12)] = ra == rbm ? 1u : 0u;
        if (blockFlagR) blockFlagR[(int64_t)brick * ((int64_t)1 << (D - 12)) + (base >> 12)] = ra == rbm ? 1u : 0u;   // half ranges all 0
    }
}

// k_pyramid12 for 16-voxel-wide boxes (ax == 4) of bricks at least 128 voxels wide: one workgroup takes the EIGHT
// x-adjacent boxes that share every 128-byte line of their rows, a 128 x 2^ay x 2^az slab of 256 rows.  Thread t loads
// the 16-byte chunk t & 7 (= box t & 7) of rows (t >> 3) + 32 k, k = 0 .. 7: a wave-instruction reads 8 rows x 128
// contiguous bytes, where k_pyramid12's reads 16 bytes of each of 64 lines, and the eight loads of a thread are all
// issued before the first is used (eight times the bytes in flight).  Everything a box writes is what k_pyramid12
// writes for it, by the same functions: a constant box (SkipBlocks builds) its 128 slots, 32 threads per box; the
// others are scattered to Morton-ordered images in LDS and reduced one after the other by all 256 threads, their
// roots behind one last barrier.  A group of eight constant boxes never touches the images.
#ifndef VR_PYR_LINES_IMAGE_BOXES
#define VR_PYR_LINES_IMAGE_BOXES 8      // boxes held in LDS at once: 8, or 4 (two rounds); DESIGN.md 3.2
#endif
// the images lie 16 bytes further apart than they are long: the lanes t & 7 of one row then store to eight different
// groups of four banks, not all to one
#define PYR_LINES_IMAGE_STRIDE (4096 + 16)

__global__ void __launch_bounds__(256)
k_pyramid12_lines(Geom g, Pyr12Geom pg, const uint8_t *__restrict__ vox, uint8_t *__restrict__ temp, int64_t heapStride,
                  uint8_t *__restrict__ tempRange, uint8_t *__restrict__ outMin, uint8_t *__restrict__ outMax,
                  int64_t outStride, uint8_t *__restrict__ blockFlag, uint8_t *__restrict__ blockFlagR)
{
    constexpr int NB = VR_PYR_LINES_IMAGE_BOXES;
    static_assert(NB == 8 || NB == 4, "images per round");
    __shared__ __attribute__((aligned(16))) uint8_t leaf[NB * PYR_LINES_IMAGE_STRIDE];
    __shared__ uint32_t boxConst[4][8];     // [wave][box]: the byte x 4 all its rows of the box hold, or 0x100
    __shared__ uint32_t waveMM[8][4];       // [box][wave]
    const int brick = blockIdx.y, D = g.D;
    const int t = threadIdx.x, lane = t & 63, c = t & 7;
    // which group: group coordinates (x fastest) from shifts, as k_pyramid12's box coordinates; nbx / 8 groups in a row
    const uint32_t gid = blockIdx.x;
    const int lgx = pg.lnbx - 3;
    const int gx = (int)((gid & ((1u << lgx) - 1u)) << 7), by = (int)(((gid >> lgx) & ((1u << pg.lnby) - 1u)) << pg.ay),
              bz = (int)((gid >> (lgx + pg.lnby)) << pg.az);
    const int ymask = (1 << pg.ay) - 1;
    const uint8_t *src = vox + (int64_t)brick * g.voxels + (gx + c * 16) + (int64_t)g.X * (by + (int64_t)g.Y * bz);
    uint4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int row = (t >> 3) + 32 * k;              // y + (z << ay) inside the slab
        v[k] = *(const uint4 *)(src + (int64_t)g.X * ((row & ymask) + (int64_t)g.Y * (row >> pg.ay)));
    }
    const uint32_t *sp = pg.spread;
    const uint32_t rowBase = sp[g.X + by] | sp[g.X + g.Y + bz];    // Morton rank of box b's origin: sp[gx + 16 b] | rowBase
    uint8_t *T = temp + (int64_t)brick * heapStride;
    uint8_t *TR = tempRange ? tempRange + (int64_t)brick * heapStride : nullptr;
    // SkipBlocks builds: the constant boxes of the group leave here, as in k_pyramid12.  A box is constant if every
    // thread's 128 bytes are one byte, the 8 threads of a wave that hold the box (lanes c, c + 8, ..) agree, and the
    // four waves do.
    uint32_t constMask = 0u;                // bit b: box b is constant (the same in every thread)
    bool myConst = false;                   // box c is
    if (blockFlag) {
        const uint32_t v0 = __builtin_amdgcn_perm(0, v[0].x, 0u);                  // byte 0 x 4
        uint32_t diff = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) diff |= (v[k].x ^ v0) | (v[k].y ^ v0) | (v[k].z ^ v0) | (v[k].w ^ v0);
        const uint32_t ref = (uint32_t)__shfl((int)v0, c);                         // of the box's first lane in my wave
        const uint64_t same = __ballot(diff == 0u && v0 == ref), boxLanes = 0x0101010101010101ull << c;
        if (lane < 8) boxConst[t >> 6][lane] = (same & boxLanes) == boxLanes ? v0 : 0x100u;   // (lane == c; 0x100: no byte x 4)
        __syncthreads();
        const uint32_t c0 = boxConst[0][c];
        myConst = c0 != 0x100u && boxConst[1][c] == c0 && boxConst[2][c] == c0 && boxConst[3][c] == c0;
        constMask = (uint32_t)__ballot(myConst) & 0xFFu;                           // lanes 0 .. 7 are boxes 0 .. 7
        if (constMask) {
            const int b = t >> 5, j = t & 31;           // 32 threads write a box's 128 slots
            const uint32_t cv = (uint32_t)__shfl((int)c0, b);
            if ((constMask >> b) & 1u) {
                const uint32_t base = sp[gx + 16 * b] | rowBase;
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    pyr12_const_slot(j + 32 * m, cv, D, base, brick, T, TR, outMin, outMax, outStride, blockFlag, blockFlagR);
            }
            if (constMask == 0xFFu) return;
        }
    }
    // Morton rank of row (t >> 3) + 32 k inside a box: rank bits are an OR over coordinate bits, and the two terms
    // share no bit of the row number
    const uint32_t rlo = sp[g.X + ((t >> 3) & ymask)] | sp[g.X + g.Y + ((t >> 3) >> pg.ay)];
    for (int h = 0; h < 8 / NB; ++h) {
        if (h) __syncthreads();                         // the round before reads its images no more
        if (!myConst && c / NB == h) {
            uint8_t *img = leaf + (c % NB) * PYR_LINES_IMAGE_STRIDE;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t r0 = rlo | sp[g.X + ((32 * k) & ymask)] | sp[g.X + g.Y + ((32 * k) >> pg.ay)];
                const uint32_t vw[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                for (int i = 0; i < 16; ++i) img[r0 | pg.sx[i]] = (uint8_t)(vw[i >> 2] >> ((i & 3) * 8));
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int b = h * NB; b < (h + 1) * NB; ++b)
            if (!((constMask >> b) & 1u))
                pyr12_reduce_box(leaf + (b % NB) * PYR_LINES_IMAGE_STRIDE, D, sp[gx + 16 * b] | rowBase, t, T, TR, waveMM[b]);
    }
    __syncthreads();
    if (t < 8 && !((constMask >> t) & 1u))
        pyr12_box_root(waveMM[t], D, sp[gx + 16 * t] | rowBase, brick, T, TR, outMin, outMax, outStride, blockFlag, blockFlagR);
}

// --------------------------------------------------------------- compress ----
struct ReconBufs { uint8_t *b[3]; };

// Constant 4096-leaf blocks (kd_encode.hip k_pyramid12 sees min == max at their depth-(D-12) root) whose depth-(D-3)
// nodes are already reconstructed exactly: every node below has truth == parent's reconstruction, so it keeps
// (code 0), reproduces the value and adds no error at ANY distance (encodeNode R.cpp:457-502 with pd = 0), and the
// running-mean estimator never counts it (R.cpp:415-455).  The level loop does not touch such a block at levels D-1 and
// D at all -- no loads, no stores; its codes and reconstruction there stay unwritten and nothing reads them: the fused
// prune/emit kernel takes the block as one pruned subtree from the flag.  flag[block]: bit 0 constant (k_pyramid12),
// bit 1 skip (set by the level D-2 fill, whose wave is exactly one block and sees truth == parents there).
struct SkipBlocks {
    uint8_t *flag;        // B * nBlk, or null: feature off (MidRangeTree, tolerance 0, small trees, general extents)
    int64_t nBlk;
    int Dm2;              // D - 2
};
__device__ __forceinline__ bool skip_block(const SkipBlocks &sk, int brick, int d, uint32_t node)
{   // node of level d (d == D-1 or D) inside a skipped block?
    return sk.flag && d > sk.Dm2 && (sk.flag[(int64_t)brick * sk.nBlk + (node >> (10 + d - sk.Dm2))] & 2u) != 0u;
}

// 1: k_fill16 fetches the skip flags of all its chunks in one batch in the prologue and walks its live chunks two loads
// deep, with no conditional memory operation in the loop.  0: the loop as it was (a flag load and a drained memory
// counter per chunk), for a trace of the old behaviour.
#ifndef VR_FLAGS_BATCHED
#define VR_FLAGS_BATCHED 1
#endif

__device__ inline int phys_buf(const Ctrl &c, int role) { return role == 0 ? c.ra : c.rb; }

// rootMin/rootMax: the pyramid's (min, max) of each brick's root, or null.  A brick whose voxels are
// all equal has a closed-form encoding (k_const_finish); every later kernel skips it.
__global__ void k_ctrl_init(Ctrl *ctrls, const uint8_t *rootMin, const uint8_t *rootMax, int64_t mmStride)
{
    Ctrl &c = ctrls[blockIdx.x];
    if (threadIdx.x) return;
    c.constBrick = 0; c.constVal = 0; c.zeroRun = 0;
    if (rootMin) {
        const int mn = rootMin[(int64_t)blockIdx.x * mmStride], mx = rootMax[(int64_t)blockIdx.x * mmStride];
        c.constBrick = mn == mx ? 1 : 0;
        c.constVal = mn;
    }
    c.currentDistance = c.currentError = c.currentDF = c.currentStepSize = 0.0; // defect C-1 pinned to zero
    c.previousDistance = c.previousError = c.previousDF = c.previousStepSize = 0.0;
    c.errMinus = c.errPlus = 0;
    c.statL1 = 0;
    c.numActive = 0;
    c.epoch = 0; c.active = 0; c.fillThisEpoch = 0;
    c.cur = 0; c.prev = 1; c.pendingEqual = 0;
    c.par = 0; c.ra = 1; c.rb = 2;
    c.altValid = 0; c.altSel = 0; c.altDist = 0;
    c.numReverts = 0; c.maxErrBefore = 0; c.maxErrAfter = 0;
    c.estS = 0; c.estC = 0; c.estT = 0; c.estUp = 0; c.estQuadFb = 0; c.estFallbacks = 0; c.estSeg = 0; c.estDone = 0; c.emitOverflow = 0;
    for (int i = 0; i < VR_MAX_DEPTH + 8; ++i) c.distanceMap[i] = 0;
}

// ---- running-mean start distance (R.cpp:254-266, encodeNodeEstimate R.cpp:415-455) ----
// The filter state (S,C) feeds back into every decision:
//     counted <=> pd>0 && ( S < pd*(2C+1) || (t>p && 2t-p>255) || (t<p && 2t<p) )      (*)
// (exact integer form of the reference's double arithmetic; S = sum of counted pd,
// C = their count, pd = |parent - truth|).  Plain fixed-point iteration over the whole
// level does not converge quickly (a flipped decision perturbs every later one), so
// the level is processed in three steps that are exact by construction:
//   k_est_head  one wave walks the first EST_HEAD nodes in order (64 nodes per step,
//               ballot iterated to its fixed point = the serial result by induction
//               on lanes) and fixes a window of EST_CAND candidate thresholds.
//   k_est_summ  fully parallel: for every later segment of EST_SEG nodes and every
//               candidate T, the sums the segment would add IF floor(S/(2C+1)) == T
//               held at every node of it (then (*) reduces to pd > T), plus two
//               bounds A,B such that the hypothesis is true for a start state (S0,C0)
//               whenever  S0 - T(2C0+1) >= A  and  S0 - (T+1)(2C0+1) < B.
//   k_est_walk  one wave carries the exact (S,C) through the segments, 64 per step:
//               prefix-sums the hypothesised sums, checks A/B for every segment with
//               its exact start state, commits up to the first failure and walks only
//               that segment node by node.
// The rounds of a level -- which segments, how wide a window, which kernel -- are est_round_plan's (host_plan.cpp):
// a 4-wide and a 2-wide prefix round, a 1-wide bulk round, a 4-wide one for the bricks that left it, then EST_CAND-wide
// exact rounds; the last round walks exactly if it must.
#define EST_SEG VR_EST_SEG
#define EST_CAND VR_EST_CAND    // widest candidate window (records hold EST_CAND entries)
#define EST_HEAD VR_EST_HEAD

// Segment summaries of one brick: one plane per candidate, 16 bytes (sumS, sumC, A, B) per segment in it.
// k_est_summ writes a candidate's record with one 16-byte store (a segment's last lane); the walking wave reads 64
// consecutive segments of its candidate as one contiguous kilobyte.
#define est_at(ci, seg) (((int64_t)(ci) * summStride + (int64_t)(seg)) * 4)

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, int lane)
{
    (void)lane;
    return wave_incl_scan_add_dpp(v);      // DPP network: no LDS-crossbar round trips in the serial walks
}

// value of a wave-uniform lane: v_readlane (a few cycles) instead of an LDS-crossbar shuffle
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ unsigned long long lane_u64(unsigned long long v, int l)
{
    return (unsigned long long)lane_u32((uint32_t)v, l) | ((unsigned long long)lane_u32((uint32_t)(v >> 32), l) << 32);
}

// exact in-order walk of nodes [lo, hi) by one wave; (S,C) are wave-uniform
#define EST_STAGE_NODES 4096        // est_exact_chain's LDS staging area holds this many truths and half as many parents
__device__ inline void est_exact_chain(const uint8_t *__restrict__ T, const uint8_t *__restrict__ P, int d, uint32_t lo,
                                       uint32_t hi, unsigned long long &S, uint32_t &C, int lane, const SkipBlocks &sk, int brick,
                                       uint8_t *stage = nullptr)
{
    // A walk is a chain of 64-node steps, each waiting for its bytes: with the next step's loads in flight it still ran at
    // one memory round trip per step (50 us for the 4096 nodes k_est_head walks on every level).  Ranges that fit are
    // staged in LDS by ONE batch of 16-byte loads (this wave is the workgroup: its LDS accesses are ordered).
    const uint32_t len = hi - lo;
    const bool staged = stage && d > 0 && len >= 64u && len <= (uint32_t)EST_STAGE_NODES && (len & 63u) == 0u && (lo & 31u) == 0u;
    const uint8_t *sT = stage, *sP = stage + EST_STAGE_NODES;
    if (staged) {
        for (uint32_t i = (uint32_t)lane * 16u; i < len; i += 1024u) *(uint4 *)(stage + i) = *(const uint4 *)(T + lo + i);
        for (uint32_t i = (uint32_t)lane * 16u; i < len / 2u; i += 1024u) *(uint4 *)(stage + EST_STAGE_NODES + i) = *(const uint4 *)(P + (lo >> 1) + i);
    }
    // the next 64 nodes are in flight while these are decided (the walk is latency-bound otherwise); chunks inside a
    // skipped block (SkipBlocks: nothing there counts, and its parents' reconstruction is not in memory) are passed over
    const bool sk0 = skip_block(sk, brick, d, lo);
    int tn = 0, pn = 0;
    if (staged) { tn = sT[lane]; pn = sP[lane >> 1]; }
    else { tn = (!sk0 && lo + lane < hi) ? T[lo + lane] : 0; pn = (!sk0 && lo + lane < hi && d > 0) ? P[(lo + lane) >> 1] : 0; }
    bool skipThis = sk0;
    for (uint32_t base = lo; base < hi; base += 64) {
        uint32_t i = base + lane;
        bool valid = i < hi;
        const int t = tn, p = pn;
        const bool skipped = skipThis;
        {
            const uint32_t i2 = i + 64;
            skipThis = base + 64 < hi && skip_block(sk, brick, d, base + 64);
            if (staged) {
                const uint32_t j2 = i2 - lo;
                tn = j2 < len ? sT[j2] : 0;
                pn = j2 < len ? sP[j2 >> 1] : 0;
            } else {
                tn = (!skipThis && i2 < hi) ? T[i2] : 0;
                pn = (!skipThis && i2 < hi && d > 0) ? P[i2 >> 1] : 0;
            }
        }
        if (skipped) continue;
        int pd = p > t ? p - t : t - p;
        bool forced = (t > p && 2 * t - p > 255) || (t < p && 2 * t < p);
        bool cand = valid && pd > 0;
        // first guess: the threshold at the chunk start
        bool dec = cand && (forced || S < (unsigned long long)pd * (2ull * C + 1ull));
        unsigned long long mask = __ballot(dec);
        for (int it = 0; it < 65; ++it) {
            uint32_t cpre = __popcll(mask & ((1ull << lane) - 1ull));
            uint32_t v = dec ? (uint32_t)pd : 0u;
            uint32_t spre = wave_incl_scan_u32(v, lane) - v;
            bool nd = cand && (forced || (S + spre) < (unsigned long long)pd * (2ull * (C + cpre) + 1ull));
            unsigned long long nmask = __ballot(nd);
            dec = nd;
            if (nmask == mask) break;
            mask = nmask;
        }
        // (a DPP scan + readlane: six dependent LDS-crossbar shuffles would cost more than the rest of the step)
        S += (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_add_dpp(dec ? (uint32_t)pd : 0u), 63);
        C += __popcll(mask);
    }
}

// where a walk stands, for the next round: the exact state, the threshold and the half of its interval the mean is in
__device__ inline void est_park(Ctrl &c, unsigned long long S, uint32_t C, uint32_t seg)
{
    const unsigned long long q = 2ull * C + 1ull, T = S / q;
    c.estS = S; c.estC = C; c.estSeg = (int)seg;
    c.estT = (int)T;
    c.estUp = 2ull * (S - T * q) >= q ? 1 : 0;
}

__device__ inline void est_finish(Ctrl &c, unsigned long long S, uint32_t C, int maxEpochs)
{
    c.currentDistance = C > 0 ? round((double)S / (double)C) : 0.0; // R.cpp:263-266
    c.previousDistance = 0.0;  // R.cpp:272-274
    c.previousStepSize = 255.0;
    c.previousError = 65025.0;
    c.epoch = 0;
    c.active = maxEpochs > 0 ? 1 : 0;
    c.fillThisEpoch = c.active;
    c.errMinus = c.errPlus = 0;
    c.cur = 0; c.prev = 1; c.pendingEqual = 0;
}

__global__ void __launch_bounds__(64)
k_est_head(int d, int maxEpochs, Ctrl *ctrls, const uint8_t *__restrict__ temp, int64_t heapStride, ReconBufs rb,
           int64_t leafStride, SkipBlocks sk)
{
    const int brick = blockIdx.x, lane = threadIdx.x;
    Ctrl &c = ctrls[brick];
    if (c.constBrick) return;
    const uint8_t *T = temp + (int64_t)brick * heapStride + ((int64_t)1 << d);
    const uint8_t *P = rb.b[c.par] + (int64_t)brick * leafStride;
    const uint32_t n = 1u << d;
    unsigned long long S = 0;
    uint32_t C = 0;
    __shared__ __attribute__((aligned(16))) uint8_t stage[EST_STAGE_NODES + EST_STAGE_NODES / 2];
    est_exact_chain(T, P, d, 0, n < EST_HEAD ? n : EST_HEAD, S, C, lane, sk, brick, stage);
    if (lane == 0) {
        if (n <= EST_HEAD) est_finish(c, S, C, maxEpochs);
        else {
            est_park(c, S, C, EST_HEAD / EST_SEG);
            c.estDone = 0;
            c.estQuadFb = 0;
        }
    }
}

// A segment's inclusive scan, maximum and minimum over its 32 lanes of the wave (two DPP rows joined by one
// row_bcast:15); the maximum and minimum are valid in the segment's last lane.
__device__ __forceinline__ uint32_t seg_incl_scan_add_dpp(uint32_t v)
{
    v = row_incl_scan_add_dpp(v);
    return v + dpp_u32<0x142, 0xa>(0, v);       // row_bcast:15 into rows 1, 3
}
__device__ __forceinline__ int seg_max_i32_dpp(int v)
{
    v = row_max_i32_dpp(v);
    return max(v, (int)dpp_u32<0x142, 0xa>(0x80000000u, (uint32_t)v));
}
__device__ __forceinline__ int seg_min_i32_dpp(int v)
{
    v = row_min_i32_dpp(v);
    return min(v, (int)dpp_u32<0x142, 0xa>(0x7FFFFFFFu, (uint32_t)v));
}

// One wave per two consecutive segments: lanes 32r .. 32r+31 summarise segment g + r, 32 consecutive nodes per lane
// as two chains of NP = 16 (nodes k and k+16 share a packed 16-bit register pair; |low| <= 16*510 and cc <= 16 per
// chain fit).  A segment's scan and extremes stay inside its two DPP rows, so the per-lane epilogue of a candidate
// serves two segments (one segment per wave and 16 nodes per lane spent a third of the candidate loop there).  Four
// segments per wave (one per row, 64 nodes per lane) need 138 VGPRs, three waves per SIMD, and measured slower.
// With h = (t>p ? 255-t : t) the reference's "forced" cases are pd > h, so under the hypothesis
// floor(S/(2C+1)) == Th node k counts  <=>  pd_k > min(Th, h_k).
//
// QUADS (the first round's kernel): sufficient bounds from byte-packed quads.  k_est_walk checks every record against
// the exact start state and walks the segment node by node when the check fails, so the sums must be exact under the
// hypothesis, but A and B only have to be SUFFICIENT: a record with A' >= A and B' <= B passes only where the exact one
// passes, and can never change a byte of the output, only cause a fallback.  The lane's 32 nodes are 8 quads of four
// consecutive nodes; once per lane and quad (candidate-independent):
//     pd4   the four pd bytes
//     hi    0x80 in each byte whose node counts under EVERY candidate Th <= 127: pd >= 128, or forced.  With
//           u = t + (t - p) in a 16-bit lane, t > p gives 0 <= u <= 510 and 2t-p > 255 <=> bit 8 of u; t < p gives
//           u < 255, and 2t < p <=> u < 0 <=> bit 8 of u; t == p gives u = t.  So bit 8 of u is "forced".
//     x7    pd4 & 0x7F7F7F7F
// and per candidate  ind = ((x7 + (0x7F - Th) * 0x01010101) & 0x80808080) | hi : 0x80 where the node counts.  x7 <= 127
// and 0x7F - Th <= 127 for 0 <= Th <= 127: no byte carries into its neighbour, and bit 7 of a byte's sum is set
// <=> x7 + 127 - Th >= 128 <=> x7 > Th.  A node with pd >= 128 > Th is in hi.  Forced and pd > Th both imply pd > 0, so
// the clamp term h needs no case of its own.  No reachable threshold is above 127 (every counted pd <= 255, so
// S / (2C + 1) < 127.5): such a candidate's record is written to fail always (A = INT_MAX).
// The sums are dot products, scaled by 128: s128 = udot4(ind, pd4, s128), cc128 = udot4(ind, 0x01010101, cc128).
// The extremes are taken from the state BEFORE each quad (on the scaled accumulators, unscaled by an exact >> 7):
//     A_q = max over quad starts of 2 Th cc - s,         B_q = min over quad starts of 2 (Th + 1) cc - s.
// A position inside a quad differs from the quad's start by at most three counted nodes.  A counted node adds
// 2 Th - pd to `low`: at most Th - 1 if it is not forced (pd > Th), at most 2 Th - 1 if it is (pd >= 1); it adds
// 2 Th + 2 - pd >= 2 Th + 2 - pdmax to `low + 2 cc`, pdmax the lane's largest pd.  Hence, per lane,
//     A' = A_q + 3 max(anyForcedInLane ? 2 Th - 1 : Th - 1, 0) >= A,      B' = B_q - 3 max(pdmax - 2 Th - 2, 0) <= B
// and the cross-lane epilogue (offsets by the exact sums of the lanes before) keeps both inequalities.  (Bounds exact
// only at lane granularity had a slack of ~100 against a true excursion of ~10 and failed almost every segment of a
// brick near a threshold boundary; here it is a handful of units.)  Lane-uniform waves keep their closed form, which
// is exact.  8 instructions per quad and candidate instead of 9 per node pair.
template <bool QUADS>
__global__ void __launch_bounds__(256)
k_est_summ(int d, int nc, uint32_t segEnd, int budget, Ctrl *ctrls, const uint8_t *__restrict__ temp, int64_t heapStride, ReconBufs rb,
           int64_t leafStride, uint32_t *__restrict__ summ, int64_t summStride, SkipBlocks sk)
{
    constexpr int L = 32, SPW = 64 / L, NP = EST_SEG / 2 / L, TW = NP / 2, PW = NP / 4;   // lanes and pairs per segment, words per lane
    const int brick = blockIdx.y, lane = threadIdx.x & 63, row = lane / L, rl = lane % L;
    const Ctrl &c = ctrls[brick];
    // one scalar round trip for the control-block fields, in front of the first branch
    const int cConst = c.constBrick, cDone = c.estDone, cSeg = c.estSeg, cPar = c.par, cT = c.estT, cUp = c.estUp, cFb = c.estQuadFb;
    // (budget >= 0, a quad round: a brick that has spent its level's budget waits for the exact rounds, as k_est_walk does)
    if (cConst || cDone || (budget >= 0 && cFb > budget)) return;
    // this round's segments end at segEnd (the level's end or before it): the records behind it are not written, and
    // k_est_walk reads none of them.  Below, `nseg` is that end
    const uint32_t nseg = segEnd;
    // segments from where the walk stands (any start, not a multiple of SPW); later rounds run on a small grid
    const uint8_t *Tl = temp + (int64_t)brick * heapStride + ((int64_t)1 << d) + rl * (4 * TW);
    const uint8_t *Pl = (cPar == 0 ? rb.b[0] : (cPar == 1 ? rb.b[1] : rb.b[2])) + (int64_t)brick * leafStride + rl * (4 * PW);
    const uint32_t step = gridDim.x * (4u * SPW);
    const uint32_t g0 = (uint32_t)cSeg + (blockIdx.x * 4u + (threadIdx.x >> 6)) * SPW;
    // the next segments' bytes are in flight while these are summarised (a wave's load round trip is what bounds
    // this kernel otherwise).  A segment past the round's end or inside a skipped block (SkipBlocks) loads nothing:
    // its zero bytes are pd = 0 everywhere, which never counts and yields the all-zero record by itself.
    uint4 tN[TW / 4], pN[PW / 4];
    auto fetch = [&](uint32_t g) {
        const uint32_t s = g + (uint32_t)row;
        const bool live = s < nseg && !skip_block(sk, brick, d, s * EST_SEG);
#pragma unroll
        for (int j = 0; j < TW / 4; ++j) tN[j] = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < PW / 4; ++j) pN[j] = make_uint4(0, 0, 0, 0);
        if (live) {
#pragma unroll
            for (int j = 0; j < TW / 4; ++j) tN[j] = ld16(Tl + (size_t)s * EST_SEG + 16 * j);
#pragma unroll
            for (int j = 0; j < PW / 4; ++j) pN[j] = ld16(Pl + (size_t)s * (EST_SEG / 2) + 16 * j);
        }
    };
    fetch(g0);
    const int Tbase = est_window_base(cT, cUp, nc);
    uint32_t *out = summ + (int64_t)brick * summStride * (4 * EST_CAND);
    for (uint32_t g = g0; g < nseg; g += step) {
    uint32_t tw[TW], pw[PW];
#pragma unroll
    for (int j = 0; j < TW / 4; ++j) { tw[4 * j] = tN[j].x; tw[4 * j + 1] = tN[j].y; tw[4 * j + 2] = tN[j].z; tw[4 * j + 3] = tN[j].w; }
#pragma unroll
    for (int j = 0; j < PW / 4; ++j) { pw[4 * j] = pN[j].x; pw[4 * j + 1] = pN[j].y; pw[4 * j + 2] = pN[j].z; pw[4 * j + 3] = pN[j].w; }
    const uint32_t seg = g + (uint32_t)row;
    const bool segLive = seg < nseg;         // segments past the round's end store nothing
    // Lane-uniform waves (both segments): every lane's 32 truths are one value and its 16 parents' reconstructions one
    // value -- constant 4096-leaf blocks below their root, see k_fill16.  All pairs of the lane are pair 0 then, and the
    // candidate loop below has a closed form.
    uint32_t mixed = 0;
    {
        const uint32_t t0 = __builtin_amdgcn_perm(0, tw[0], 0u), p0 = __builtin_amdgcn_perm(0, pw[0], 0u);   // byte 0 x 4
#pragma unroll
        for (int j = 0; j < TW; ++j) mixed |= tw[j] ^ t0;
#pragma unroll
        for (int j = 0; j < PW; ++j) mixed |= pw[j] ^ p0;
    }
    const bool uniform = __ballot(mixed != 0u) == 0ull;
    constexpr int NU = QUADS ? 1 : NP, NQ = QUADS ? TW : 1;      // QUADS unpacks pair 0 only (lane-uniform waves)
    vr_s16x2 pd[NU], h[NU];
    uint32_t anyPd = 0;
    uint32_t pd4[NQ], hi[NQ], anyF = 0;                  // QUADS: see the header comment
    vr_s16x2 pm = (vr_s16x2)(0);
    const auto unpack4 = [&](const int q) {
        // nodes 4q .. 4q+3: even and odd bytes of the truth word share the parents (byte 2q, byte 2q+1)
        const uint32_t psel = (uint32_t)((2 * q) & 3);
        const vr_s16x2 P2 = pk_s(__builtin_amdgcn_perm(0, pw[q >> 1], 0x0c000c00u | psel | ((psel + 1u) << 16)));
        const vr_s16x2 Te = pk_s(__builtin_amdgcn_perm(0, tw[q], 0x0c020c00u)), To = pk_s(__builtin_amdgcn_perm(0, tw[q], 0x0c030c01u));
        const vr_s16x2 de = Te - P2, dO = To - P2;
        const vr_s16x2 pe = __builtin_elementwise_max(de, (vr_s16x2)(0) - de), po = __builtin_elementwise_max(dO, (vr_s16x2)(0) - dO);
        const uint32_t fb = __builtin_amdgcn_perm(pk_u(To + dO), pk_u(Te + de), 0x07030501u);     // bit 0 of each byte: forced
        pd4[q] = __builtin_amdgcn_perm(pk_u(po), pk_u(pe), 0x06020400u);
        hi[q] = ((fb << 7) | pd4[q]) & 0x80808080u;
        anyF |= fb;
        pm = __builtin_elementwise_max(pm, __builtin_elementwise_max(pe, po));
    };
    const auto unpack = [&](const int k) {
        // lanes: (node k, node k+NP); their parents are bytes k>>1 and NP/2 + (k>>1) of the lane's parent bytes
        const uint32_t bsel = (uint32_t)(k & 3), psel = (uint32_t)((k >> 1) & 3);
        const uint32_t T2 = __builtin_amdgcn_perm(tw[(k >> 2) + TW / 2], tw[k >> 2], 0x0c040c00u | bsel | (bsel << 16));
        const uint32_t P2 = __builtin_amdgcn_perm(pw[(k >> 3) + PW / 2], pw[k >> 3], 0x0c040c00u | psel | (psel << 16));
        const vr_s16x2 diff = pk_s(T2) - pk_s(P2), nd = (vr_s16x2)(0) - diff;
        pd[k] = __builtin_elementwise_max(diff, nd);
        h[k] = pk_s(T2 ^ (pk_u(nd >> 15) & 0x00FF00FFu));
        anyPd |= pk_u(pd[k]);
    };
    if (uniform) unpack(0);
    else if constexpr (QUADS) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) unpack4(q);
        anyPd = pk_u(pm);
    } else
#pragma unroll
        for (int k = 0; k < NP; ++k) unpack(k);
    fetch(g + step);                         // after the unpacking: these bytes and those loads are not live together
    if (__ballot(anyPd != 0) == 0ull) {      // parents reproduce the truths exactly in all segments (constant regions)
        if (segLive && rl < nc) *(uint4 *)(out + est_at(rl, seg)) = make_uint4(0, 0, 0, 0);
        continue;
    }
    // every h of the wave at or above the last candidate (the usual case away from 0 and 255): min(Th, h) = Th
    vr_s16x2 hmin = h[0];
    if (!uniform)
#pragma unroll
        for (int k = 1; k < NU; ++k) hmin = __builtin_elementwise_min(hmin, h[k]);
    const bool hBig = !QUADS && !uniform && __ballot(min((int)hmin.x, (int)hmin.y) < Tbase + nc - 1) == 0ull;
    const int pdmax = max((int)pm.x, (int)pm.y), forcedLane = (anyF & 0x01010101u) != 0u ? 1 : 0;
#pragma unroll 1
    for (int ci = 0; ci < nc; ++ci) {
        const int Th = Tbase + ci;
        int a, b, lowT, ccT;
        if (QUADS && Th > 127) {             // unreachable threshold: a record that always fails
            if (segLive && rl == L - 1) *(uint4 *)(out + est_at(ci, seg)) = make_uint4(0, 0, 0x7FFFFFFFu, 0x7FFFFFFFu);
            continue;
        }
        if (QUADS && !uniform) {
            const uint32_t kadd = (uint32_t)(0x7F - Th) * 0x01010101u;
            const int m2 = -2 * Th, m22 = -2 * Th - 2;
            uint32_t s128 = 0, cc128 = 0;
            int mn = 0, mx = 0;              // min of s - 2 Th cc (= -A_q) and max of s - 2 (Th + 1) cc (= -B_q), x 128
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (q > 0) {
                    mn = min(mn, __mul24((int)cc128, m2) + (int)s128);
                    mx = max(mx, __mul24((int)cc128, m22) + (int)s128);
                }
                const uint32_t ind = (((pd4[q] & 0x7F7F7F7Fu) + kadd) & 0x80808080u) | hi[q];
                s128 = __builtin_amdgcn_udot4(ind, pd4[q], s128, false);
                cc128 = __builtin_amdgcn_udot4(ind, 0x01010101u, cc128, false);
            }
            ccT = (int)(cc128 >> 7);
            lowT = 2 * Th * ccT - (int)(s128 >> 7);
            a = -(mn >> 7) + 3 * max(forcedLane ? 2 * Th - 1 : Th - 1, 0);
            b = -(mx >> 7) - 3 * max(pdmax - 2 * Th - 2, 0);
        } else {
        const vr_s16x2 Th2 = pk_s((uint32_t)Th * 0x10001u), w2 = pk_s((uint32_t)(2 * Th) * 0x10001u);
        // per chain: low = 2*Th*cc - s, and the extremes of low / low + 2cc over the positions BEFORE each node
        vr_s16x2 low = (vr_s16x2)(0), cc = (vr_s16x2)(0), amax = (vr_s16x2)(0), bmin = (vr_s16x2)(0);
        const vr_s16x2 two2 = pk_s(0x00020002u);
        if (uniform) {
            // All NP nodes of a chain count (pd > min(Th, h)) or none does.  With v = 2 Th - pd where they count and 0
            // where not, the chain's `low` before node j is j * v and `low + 2 cc` is j * (v + 2 [counts]): linear in
            // j, so their extremes over j = 0 .. NP-1 (what the loops below track) sit at j = 0 or j = NP - 1, and the
            // totals are NP * v and NP [counts].  |v| <= 510: NP * 512 fits 16 bits.  Equal to the chain, not a bound.
            const vr_s16x2 dm = (__builtin_elementwise_min(Th2, h[0]) - pd[0]) >> 15;     // -1 where the nodes count
            const vr_s16x2 v = pk_s(pk_u(w2 - pd[0]) & pk_u(dm)), v2 = v - dm - dm;
            low = v * (short)NP;
            cc = pk_s(pk_u(dm) & ((uint32_t)NP * 0x10001u));
            amax = __builtin_elementwise_max(amax, low - v);
            bmin = __builtin_elementwise_min(bmin, v2 * (short)NP - v2);
        } else if (hBig) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const vr_s16x2 dm = (Th2 - pd[k]) >> 15, one = pk_s(pk_u(dm) & 0x00010001u);   // -1 / 1 where the node counts
            low = one * (w2 - pd[k]) + low;         // not the other branch's expression: hoisted above the branch, it
            cc += one;                              // held NP more registers across it
            if (k < NP - 1) {
                amax = __builtin_elementwise_max(amax, low);
                bmin = __builtin_elementwise_min(bmin, pk_mad(cc, two2, low));
            }
        }
        } else
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const vr_s16x2 dm = (__builtin_elementwise_min(Th2, h[k]) - pd[k]) >> 15;     // -1 where the node counts
            low = dm * (pd[k] - w2) + low;          // += 2 Th - pd where it counts (v_pk_mad_i16)
            cc -= dm;
            if (k < NP - 1) {
                amax = __builtin_elementwise_max(amax, low);
                bmin = __builtin_elementwise_min(bmin, pk_mad(cc, two2, low));
            }
        }
        const int low1 = low.x, low2 = low.y, cc1 = cc.x, cc2 = cc.y;
        lowT = low1 + low2; ccT = cc1 + cc2;
        a = max((int)amax.x, max((int)amax.y, 0) + low1);          // chain 2 starts at position NP (its own 0 included)
        b = min((int)bmin.x, min((int)bmin.y, 0) + low1 + 2 * cc1);
        }
        const uint32_t sT = (uint32_t)(2 * Th * ccT - lowT);
        // one scan for both sums: s < 2^18 per segment, cc <= 1024
        const uint32_t packed = sT | ((uint32_t)ccT << 20);
        const uint32_t incl = seg_incl_scan_add_dpp(packed), excl = incl - packed;
        const int s0 = (int)(excl & 0xFFFFFu), c0 = (int)(excl >> 20);
        a += 2 * Th * c0 - s0;
        b += 2 * (Th + 1) * c0 - s0;
        a = seg_max_i32_dpp(a);
        b = seg_min_i32_dpp(b);
        if (segLive && rl == L - 1)      // the segment's last lane holds its totals and extremes
            *(uint4 *)(out + est_at(ci, seg)) = make_uint4(incl & 0xFFFFFu, incl >> 20, (uint32_t)a, (uint32_t)b);
    }
    }
}

// VR_EST_CENSUS (a build of its own, never the library's): k_est_walk logs every segment it walks node by node and
// where and why every round of every brick ends, for profiles/tools/est_census.py to replay against round plans.
#ifdef VR_EST_CENSUS
#define EST_CENSUS_CAP (1u << 22)
__device__ uint32_t g_estCensusN;
__device__ uint4 g_estCensus[EST_CENSUS_CAP];
enum { EC_WALKED = 1, EC_WINDOW = 2, EC_BUDGET = 3, EC_LIMIT = 4, EC_DONE = 5, EC_LAST_RESORT = 6, EC_START = 7 };    // | 256: the mean is in its interval's upper half
#define EST_UP(S_, C_, T_) (2ull * ((S_) - (unsigned long long)(T_) * (2ull * (C_) + 1ull)) >= 2ull * (C_) + 1ull ? 256u : 0u)
#define EST_LOG(kind, seg_, T_) do { if (lane == 0) { const uint32_t i_ = atomicAdd(&g_estCensusN, 1u); \
    if (i_ < EST_CENSUS_CAP) g_estCensus[i_] = make_uint4((uint32_t)brick | ((uint32_t)d << 16) | ((uint32_t)round << 24), (seg_), (uint32_t)(T_), (kind)); } } while (0)
extern "C" int64_t vr_debug_est_census(uint32_t *out, int64_t capRecords)
{
    uint32_t n = 0, zero = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_estCensusN), 4) != hipSuccess) return -1;
    const int64_t m = n < EST_CENSUS_CAP ? n : EST_CENSUS_CAP;
    if (m > capRecords) return -2;
    if (m && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_estCensus), (size_t)m * 16) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_estCensusN), &zero, 4) != hipSuccess) return -1;
    return n;
}
#else
#define EST_LOG(kind, seg_, T_) do { } while (0)
#endif

// One wave per brick.  This round's records cover the segments [c.estSeg, segEnd) under the nc thresholds from
// est_window_base(c.estT, c.estUp, nc) -- k_est_summ derives the same window from the same fields.  The walk stops where
// the threshold leaves the window, where a quad round's budget is spent, or at segEnd; short of the level's end it
// parks its state for the next round.  Records at or behind segEnd are stale: no guard below may look past it.
__global__ void __launch_bounds__(64)
k_est_walk(int d, int maxEpochs, int nc, uint32_t segEnd, int round, int lastRound, int budget, Ctrl *ctrls, const uint8_t *__restrict__ temp, int64_t heapStride, ReconBufs rb,
           int64_t leafStride, const uint32_t *__restrict__ summ, int64_t summStride, SkipBlocks sk)
{
    const int brick = blockIdx.x, lane = threadIdx.x;
    Ctrl &c = ctrls[brick];
    const uint8_t *T = temp + (int64_t)brick * heapStride + ((int64_t)1 << d);
    const uint8_t *P = rb.b[c.par] + (int64_t)brick * leafStride;
    const uint32_t n = 1u << d, nseg = n / EST_SEG;
    const uint32_t *sm = summ + (int64_t)brick * summStride * (4 * EST_CAND);
    if (c.constBrick || c.estDone) return;
    // budget >= 0 (a quad round, whose records carry sufficient bounds only): the brick's budget of node-by-node
    // segments is one per level, carried across the quad rounds; once spent, the exact rounds finish the brick
    const int fb0 = c.estQuadFb;
    if (budget >= 0 && fb0 > budget) return;
    __shared__ __attribute__((aligned(16))) uint8_t stage[EST_STAGE_NODES + EST_STAGE_NODES / 2];    // est_exact_chain's (a failed segment)
    unsigned long long S = c.estS;
    uint32_t C = c.estC;
    const int Tbase = est_window_base(c.estT, c.estUp, nc);
    long long Tc = (long long)(S / (2ull * C + 1ull));
    uint32_t seg = (uint32_t)c.estSeg;
    int fallbacks = 0;
    EST_LOG(EC_START | EST_UP(S, C, Tc), seg, Tc);
    // 256 segments per step, four consecutive ones per lane (64 contiguous bytes of its candidate's plane), the next
    // step's records in flight while these are checked (same candidate: the common case).  (64 per step, one per lane:
    // 128 steps of one memory round trip each on the leaf level, 220 us.)
    uint32_t preSeg = 0xFFFFFFFFu;
    long long preCi = -1;
    uint4 pre[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pre[j] = make_uint4(0, 0, 0x80000000u, 0x7FFFFFFFu);
    const auto fetch = [&](long long ci_, uint32_t seg_, uint4 (&r)[4]) {
        const uint32_t k0 = seg_ + 4u * (uint32_t)lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = make_uint4(0, 0, 0x80000000u, 0x7FFFFFFFu);          // (sums 0, A = INT_MIN, B = INT_MAX: always true)
            if (k0 + (uint32_t)j < segEnd) r[j] = *(const uint4 *)(sm + est_at((int)ci_, k0 + (uint32_t)j));
        }
    };
    // the next round: new summaries around the threshold of where the walk stands
    const auto park = [&]() {
        if (lane == 0) {
            est_park(c, S, C, seg);
            c.estFallbacks += fallbacks;
            if (budget >= 0) c.estQuadFb = fb0 + fallbacks;
        }
    };
    while (seg < segEnd) {
        const long long ci = Tc - Tbase;
        // a brick that has walked more than `budget` segments of the level node by node leaves the quad rounds as if
        // the threshold had left the window -- no launch lasts as long as its unluckiest brick
        const bool spent = budget >= 0 && !lastRound && fb0 + fallbacks > budget;
        if (ci < 0 || ci >= nc || spent) {   // threshold left the candidate window
            if (!lastRound) {
                EST_LOG(spent ? EC_BUDGET : EC_WINDOW, seg, Tc);
                park();
                return;
            }
            EST_LOG(EC_LAST_RESORT, seg, Tc);
            est_exact_chain(T, P, d, seg * EST_SEG, n, S, C, lane, sk, brick);   // last resort: walk the rest in order
            fallbacks += (int)(nseg - seg);
            seg = nseg;
            break;
        }
        uint4 r[4];
        if (preSeg == seg && preCi == ci) {
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = pre[j];
        } else fetch(ci, seg, r);
        preSeg = seg + 256u; preCi = ci;
        fetch(ci, preSeg, pre);
        const uint32_t k0 = seg + 4u * (uint32_t)lane;
        const uint32_t ssL = r[0].x + r[1].x + r[2].x + r[3].x, scL = r[0].y + r[1].y + r[2].y + r[3].y;
        const uint32_t si = wave_incl_scan_u32(ssL, lane), sci = wave_incl_scan_u32(scL, lane);
        uint32_t eS = si - ssL, eC = sci - scL;              // sums of the segments before mine in this step
        int failJ = 4;
        uint32_t fS = 0, fC = 0;                             // ... and before my first failing segment
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long S0 = (long long)S + (long long)eS;
            const long long q = 2ll * ((long long)C + (long long)eC) + 1ll;
            const bool ok = k0 + (uint32_t)j >= segEnd || (S0 - Tc * q >= (long long)(int)r[j].z && S0 - (Tc + 1) * q < (long long)(int)r[j].w);
            if (!ok && failJ == 4) { failJ = j; fS = eS; fC = eC; }
            eS += r[j].x; eC += r[j].y;
        }
        const unsigned long long bad = __ballot(failJ < 4);
        if (bad == 0ull) {
            S += lane_u32(si, 63);
            C += lane_u32(sci, 63);
            seg = seg + 256u < segEnd ? seg + 256u : segEnd;
            continue;
        }
        const int f = __ffsll((long long)bad) - 1;            // the lane of the first segment whose hypothesis fails
        S += lane_u32(fS, f);
        C += lane_u32(fC, f);
        seg += 4u * (uint32_t)f + lane_u32((uint32_t)failJ, f);
        est_exact_chain(T, P, d, seg * EST_SEG, (seg + 1) * EST_SEG, S, C, lane, sk, brick, stage);
        Tc = (long long)(S / (2ull * C + 1ull));
        seg += 1;
        ++fallbacks;
        EST_LOG(EC_WALKED | EST_UP(S, C, Tc), seg - 1u, Tc);
    }
    if (seg < nseg) {                        // this round's limit (the host's last round ends at the level's end)
        EST_LOG(EC_LIMIT, seg, Tc);
        park();
        return;
    }
    EST_LOG(EC_DONE, seg, Tc);
    if (lane == 0) { est_finish(c, S, C, maxEpochs); c.estFallbacks += fallbacks; c.estDone = 1; }
}

__device__ inline unsigned long long block_sum_u64(unsigned long long v, unsigned long long *sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    unsigned long long r = 0;
    if (threadIdx.x == 0) for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
    __syncthreads();
    return r; // valid in thread 0
}

// One gradient-descent evaluation of a level (R.cpp:307-313 fused with :336-359):
// writes the 2-bit code and the reconstruction at `current`, and accumulates err^2 at
// current (per-block partials, summed in node order by k_control to reproduce the
// reference's serial double sum) and at current-1 / current+1 (exact integer atomics).
__global__ void __launch_bounds__(256)
k_fill(int d, Ctrl *ctrls, const uint8_t *__restrict__ temp, uint8_t *__restrict__ codes, int64_t heapStride,
       int64_t codeStride, ReconBufs rb, int64_t leafStride, unsigned long long *__restrict__ blockErr, int64_t nErrBlk)
{
    __shared__ unsigned long long sh[4];
    const int brick = blockIdx.y;
    Ctrl &c = ctrls[brick];
    if (c.constBrick || !c.fillThisEpoch) return;
    const uint32_t n = 1u << d;
    const uint8_t *T = temp + (int64_t)brick * heapStride + ((int64_t)1 << d);
    uint8_t *Cb = codes + (int64_t)brick * codeStride;
    const uint8_t *P = rb.b[c.par] + (int64_t)brick * leafStride;
    uint8_t *R = rb.b[phys_buf(c, c.cur)] + (int64_t)brick * leafStride;
    const int dist = (int)(uint8_t)c.currentDistance;
    const int distM = (int)(uint8_t)fmax(0.0, c.currentDistance - 1.0);   // R.cpp:334
    const int distP = (int)(uint8_t)fmin(255.0, c.currentDistance + 1.0);
    unsigned long long e0 = 0, em = 0, ep = 0;
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    uint32_t pk = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t i = i0 + k;
        if (i < n) {
            int t = T[i];
            int p = d > 0 ? P[i >> 1] : 0;
            Enc e = encode_node(t, p, dist);
            pk |= (uint32_t)e.code << (2 * k);
            R[i] = (uint8_t)e.recon;
            e0 += (unsigned)(e.err * e.err);
            int a = encode_node(t, p, distM).err, b = encode_node(t, p, distP).err;
            em += (unsigned)(a * a);
            ep += (unsigned)(b * b);
        }
    }
    if (i0 < n) {
        if (d >= 2) Cb[(((int64_t)1 << d) + i0) >> 2] = (uint8_t)pk;     // four codes = one whole byte
        else if (d == 0) Cb[0] = (uint8_t)((Cb[0] & ~0x0Cu) | (pk << 2));            // heap node 1 (only writer)
        else Cb[0] = (uint8_t)((Cb[0] & 0x0Fu) | ((pk & 0xFu) << 4));                 // heap nodes 2, 3
    }
    e0 = block_sum_u64(e0, sh);
    em = block_sum_u64(em, sh);
    ep = block_sum_u64(ep, sh);
    if (threadIdx.x == 0) {
        blockErr[(int64_t)brick * nErrBlk + blockIdx.x] = e0;
        if (em) atomicAdd(&c.errMinus, em);
        if (ep) atomicAdd(&c.errPlus, ep);
    }
}

// Vector form of k_fill for levels with >= 4096 nodes: 16 consecutive nodes per thread
// (one 16-byte load of truths, one 8-byte load of parents, 16-byte stores of codes and
// reconstructions); a wave covers exactly one 1024-node partial-sum block of k_control.
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// A sibling pair of leaves as the level loop of a leafless build left it (k_prune_emit12): truth minus reconstruction at
// the distance of the buffer the loop ended on, codes at the distance of the last fill.  The two differ after a reverted
// epoch: the reference restores the reconstruction, not the codes (SURVEY C-2).  Same reduced encodeNode as k_fill16.
__device__ __forceinline__ void leaf_pair_encode(uint32_t tword, int tsel, uint32_t pword, int psel, uint32_t dR2, uint32_t dC2,
                                                 vr_s16x2 &dl, uint32_t &codes2)
{
    const EncPair c = enc_pair(tword, tsel, pword, psel);
    const vr_s16x2 x = enc_pair_x(c, dR2), nx = (vr_s16x2)(0) - x, ax = __builtin_elementwise_max(x, nx);
    uint32_t take = pk_u((ax - c.pd) >> 15);                                 // 0xFFFF per lane where |x| < pd: the step is taken
    // reconstruction = up ? t + x : t - x where taken, the parent's otherwise
    const uint32_t stepD = (c.up & pk_u(nx)) | (~c.up & pk_u(x));
    dl = pk_s((take & stepD) | (~take & pk_u(c.T2 - c.P2)));
    if (dC2 != dR2) {                                                        // (uniform per brick)
        const vr_s16x2 xc = enc_pair_x(c, dC2);
        take = pk_u((pk_abs(xc) - c.pd) >> 15);
    }
    codes2 = take & pk_u(pk_s(c.up) + pk_s(0x00020002u));                   // up ? 1 : 2 (per-lane wrap)
}

static_assert(FILL_ITERS < 32, "k_fill16 keeps a workgroup's chunks as the bits of a 32-bit mask and the lanes of a wave");
template <bool STORE>     // false (the leaf level of a leafless build): errors only -- k_prune_emit12 recomputes codes and reconstruction
__global__ void __launch_bounds__(256)
k_fill16(int d, int maxEpochs, Ctrl *ctrls, const uint8_t *__restrict__ temp, uint8_t *__restrict__ codes, int64_t heapStride,
         int64_t codeStride, ReconBufs rb, int64_t leafStride, unsigned long long *__restrict__ blockErr, int64_t nErrBlk,
         SkipBlocks sk, int64_t errPlane, int iters)
{
    // A workgroup takes `iters` consecutive chunks of 4096 nodes (a wave: 1024 = one partial-sum block of k_control),
    // the next chunk's loads in flight while this one is evaluated: two million four-wave workgroups at the leaf level
    // spent a third of the launch being dispatched and reading the control block (a level-D fill in which every wave
    // skipped took 0.94 ms).
    __shared__ unsigned long long shm[4], shp[4];
    const int brick = blockIdx.y, lane = threadIdx.x & 63;
#if VR_FLAGS_BATCHED
    // The flag bytes of all my wave's chunks in one batch (lane j: chunk j of the workgroup), in flight beside the
    // control block: at level D-2 bit 0 of my own block's byte (the pyramid's), below it bit 1 of the block above the
    // chunk, which its own wave wrote at level D-2 and nobody changes after that level.  A flag load in front of
    // every chunk's prefetch was a dependent round trip per chunk.
    uint32_t flagByte = 0;
    if (sk.flag && d >= sk.Dm2) {
        const uint32_t nch = (uint32_t)(((size_t)1 << d) >> 12), cj = blockIdx.x * (uint32_t)iters + (uint32_t)lane;
        if (lane < iters && cj < nch) flagByte = sk.flag[(int64_t)brick * sk.nBlk + ((cj * 4u + (threadIdx.x >> 6)) >> (d - sk.Dm2))];
    }
#endif
    // everything the wave needs from the brick's control block is fetched in ONE scalar round trip, before the
    // first branch (field by field behind branches it was seven dependent ones in front of the data loads)
    Ctrl &c = ctrls[brick];
    const int cConst = c.constBrick, cFill = c.fillThisEpoch, cPar = c.par, cCur = c.cur, cRa = c.ra, cRb = c.rb, cEpoch = c.epoch;
    const double cDist = c.currentDistance;
    if (cConst || !cFill) return;
    if (!STORE && c.altSel) return;          // this epoch's partials exist already (Ctrl::altSel)
    const uint8_t *T = temp + (int64_t)brick * heapStride + ((int64_t)1 << d);
    uint8_t *Cd = codes + (int64_t)brick * codeStride + ((int64_t)1 << (d - 2));   // packed: 4 codes per byte
    const int rPhys = cCur == 0 ? cRa : cRb;                                         // phys_buf(c, c.cur)
    const uint8_t *P = (cPar == 0 ? rb.b[0] : (cPar == 1 ? rb.b[1] : rb.b[2])) + (int64_t)brick * leafStride;
    uint8_t *R = (rPhys == 0 ? rb.b[0] : (rPhys == 1 ? rb.b[1] : rb.b[2])) + (int64_t)brick * leafStride;
    const int dist = (int)(uint8_t)cDist;
    const int distM = (int)(uint8_t)fmax(0.0, cDist - 1.0);   // R.cpp:334
    const int distP = (int)(uint8_t)fmin(255.0, cDist + 1.0);
    // the central difference (R.cpp:333-362) only steers a FOLLOWING epoch: in the last one its result is
    // never read (VolumeKdtree.cpp:333 skips it outright), so the two extra evaluations are not made
    const bool needDF = cEpoch + 1 < maxEpochs;
    const uint32_t d2 = (uint32_t)dist * 0x10001u, dm2 = (uint32_t)distM * 0x10001u, dp2 = (uint32_t)distP * 0x10001u;
    const int w = threadIdx.x >> 6;
    const uint32_t nchunk = (uint32_t)(((size_t)1 << d) >> 12);
    uint32_t chunk = blockIdx.x * (uint32_t)iters;
    const uint32_t chunkEnd = chunk + (uint32_t)iters < nchunk ? chunk + (uint32_t)iters : nchunk;
    unsigned long long accM = 0, accP = 0;
#if VR_FLAGS_BATCHED
    const uint32_t skipMask = d > sk.Dm2 ? (uint32_t)__ballot((flagByte & 2u) != 0u) : 0u;
    const uint32_t constMask = d == sk.Dm2 ? (uint32_t)__ballot((flagByte & 1u) != 0u) : 0u;
#endif
    // One chunk of my wave (1024 nodes, 16 per lane): codes and reconstruction words of the lane, the wave's err^2 sums
    // at the three distances, and whether any truth differs from its parent's reconstruction.
    const auto eval = [&](const uint4 tv, const uint2 pv, const bool skipped, uint32_t &cpk, uint32_t (&rw)[4], uint32_t &s0,
                          uint32_t &sm, uint32_t &sp) -> bool {
    const uint32_t tw[4] = {tv.x, tv.y, tv.z, tv.w}, pw[2] = {pv.x, pv.y};
    uint32_t e0 = 0, em = 0, ep = 0, wa = 0, wb = 0, rprev = 0;
    rw[0] = tw[0]; rw[1] = tw[1]; rw[2] = tw[2]; rw[3] = tw[3];
    // a wave whose 1024 truths all equal their parents' reconstruction (constant regions) has nothing to decide:
    // every code is "keep", the reconstruction is the truth, the error 0 at any distance (pd = 0 in encodeNode)
    const uint32_t differs = (tw[0] ^ __builtin_amdgcn_perm(0, pw[0], 0x01010000u)) | (tw[1] ^ __builtin_amdgcn_perm(0, pw[0], 0x03030202u)) |
                             (tw[2] ^ __builtin_amdgcn_perm(0, pw[1], 0x01010000u)) | (tw[3] ^ __builtin_amdgcn_perm(0, pw[1], 0x03030202u));
    const bool busy = !skipped && __ballot(differs != 0u) != 0ull;
    const auto pair = [&](const int j) {                 // sibling pair j: nodes 2j, 2j+1, parent byte j
        const EncPair c = enc_pair(tw[j >> 1], j & 1, pw[j >> 2], j & 3);
        const vr_s16x2 x = enc_pair_x(c, d2), ax = pk_abs(x);
        e0 = pk_sumsq(__builtin_elementwise_min(c.pd, ax), e0);
        if (STORE) {
        const uint32_t take = pk_u((ax - c.pd) >> 15);                 // 0xFFFF per lane where |x| < pd
        const uint32_t code2 = take & pk_u(pk_s(c.up) + pk_s(0x00020002u));   // up ? 1 : 2 (per-lane wrap)
        if (j < 4) wa |= code2 << (4 * j); else wb |= code2 << (4 * (j - 4));
        const vr_s16x2 r = pk_mad(x, pk_mad(pk_s(c.up), pk_s(0xFFFEFFFEu), pk_s(0xFFFFFFFFu)), c.T2);   // up ? t + x : t - x  (sign = -2 up - 1)
        const uint32_t rec = (take & pk_u(r)) | (~take & pk_u(c.P2));
        if (j & 1) rw[j >> 1] = __builtin_amdgcn_perm(rec, rprev, 0x06040200u); else rprev = rec;
        }
        if (needDF) {
            em = pk_sumsq(enc_pair_err(c, dm2), em);
            ep = pk_sumsq(enc_pair_err(c, dp2), ep);
        }
    };
    // Lane-uniform waves: every lane's 16 truths are one value and its 8 parents' reconstructions one value (lanes
    // differ freely).  Inside a constant 4096-leaf block that is every lane of every level below the block's root, by
    // induction: equal truths and equal parents give equal reconstructions.  The lane's eight pairs are then the same
    // computation: pair 0 is evaluated, its reconstruction byte and code replicated, and its err^2 (integers, so the
    // lane's sum is exactly eight times the pair's) multiplied.  The exact shortcut above stays in front (cheaper still).
    bool uniform = false;
    if (busy) {
        const uint32_t t0 = __builtin_amdgcn_perm(0, tw[0], 0u), p0 = __builtin_amdgcn_perm(0, pw[0], 0u);   // byte 0 x 4
        const uint32_t mixed = (tw[0] ^ t0) | (tw[1] ^ t0) | (tw[2] ^ t0) | (tw[3] ^ t0) | (pw[0] ^ p0) | (pw[1] ^ p0);
        uniform = __ballot(mixed != 0u) == 0ull;
    }
    if (uniform) {
        pair(0);
        e0 *= 8u; em *= 8u; ep *= 8u;
        if (STORE) {
            wa *= 0x1111u; wb = wa;                      // pair 0's codes (bits 0-1 and 16-17) at every pair slot
            rw[0] = rw[1] = rw[2] = rw[3] = __builtin_amdgcn_perm(0, rprev, 0u);
        }
    } else if (busy)
#pragma unroll
        for (int j = 0; j < 8; ++j) pair(j);
    // even nodes sit at bits 4j, odd ones at 16+4j: fold to 2 bits per node
    cpk = ((wa | (wa >> 14)) & 0xFFFFu) | ((wb | (wb >> 14)) << 16);
    // per-lane sums are < 2^21, a wave's < 2^27: 32-bit DPP scans, the total in lane 63
    s0 = sm = sp = 0;
    if (busy) {
        s0 = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_add_dpp(e0), 63);
        sm = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_add_dpp(em), 63);
        sp = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_add_dpp(ep), 63);
    }
    return busy;
    };
#if VR_FLAGS_BATCHED
    // Chunk j of the workgroup is bit j and lane j.  The loop below visits my wave's live chunks only (a skipped one:
    // no error, nothing to load, nothing anybody will read) and holds no conditional memory operation: two chunks of
    // inputs are in flight, a chunk's registers are refilled as soon as it is evaluated and stored (with the refill in
    // front of the stores the compiler loads into fresh registers and copies them at the back edge, behind a wait), and
    // every wait on them counts the younger operations instead of draining the counter.  Where the live chunks run out
    // the refill reads one line the wave has just read, for nobody.  The per-chunk sums wait in lane j's registers and
    // the level D-2 flag bits in a mask; both are stored once, after the loop.
    const uint32_t cnt = chunkEnd - chunk, liveMask = ((1u << cnt) - 1u) & ~skipMask;
    uint32_t errS = 0, errM = 0, errP = 0, exactMask = 0;
    if (liveMask) {
        uint32_t m = liveMask;
        const size_t idle = ((size_t)(chunk + (31u - (uint32_t)__builtin_clz(liveMask))) * 256u + (size_t)(w << 6)) * 16u;
        int kA, kB;
        uint4 tA, tB;
        uint2 pA, pB;
        const auto next = [&](int &k, uint4 &tv, uint2 &pv) {
            k = m ? __builtin_ctz(m) : -1;
            m &= m - 1u;
            const size_t i = k >= 0 ? ((size_t)(chunk + (uint32_t)k) * 256u + threadIdx.x) * 16u : idle;
            tv = ld16(T + i); pv = ld8(P + (i >> 1));
        };
        const auto phase = [&](int &k, uint4 &tv, uint2 &pv) {
            const int kc = k;
            const size_t i0 = ((size_t)(chunk + (uint32_t)kc) * 256u + threadIdx.x) * 16u;
            uint32_t cpk, rw[4], s0, sm, sp;
            const bool busy = eval(tv, pv, false, cpk, rw, s0, sm, sp);
            if (STORE) {
                st4(Cd + (i0 >> 2), cpk);
                st16(R + i0, make_uint4(rw[0], rw[1], rw[2], rw[3]));
            }
            next(k, tv, pv);
            if (lane == kc) { errS = s0; errM = sm; errP = sp; }
            accM += sm; accP += sp;
            if (!busy) exactMask |= 1u << kc;
        };
        next(kA, tA, pA);
        next(kB, tB, pB);
        phase(kA, tA, pA);
        // (the loop's head sits behind the first evaluation, so that both ways into it have A's refill and stores
        // behind B's loads)
        while (kB >= 0) {
            phase(kB, tB, pB);
            if (kA < 0) break;
            phase(kA, tA, pA);
        }
    }
    if ((uint32_t)lane < cnt) {
        const int64_t at = (int64_t)brick * nErrBlk + (size_t)(chunk + (uint32_t)lane) * 4 + w;     // 1024 nodes per wave
        blockErr[at] = errS;
        if (!STORE && needDF) {     // the central difference's sums per block too: a following epoch at distance -1 / +1 is these
            blockErr[errPlane + at] = errM;
            blockErr[2 * errPlane + at] = errP;
        }
        // level D-2: my wave IS one 4096-leaf block's nodes of this level.  Constant block (k_pyramid12) and every truth
        // equal to its parent's reconstruction: the two levels below need not be visited (SkipBlocks).  The same answer
        // in every epoch of the level: it depends on truths and parents only.
        if (((exactMask & constMask) >> lane) & 1u) sk.flag[(int64_t)brick * sk.nBlk + (size_t)(chunk + (uint32_t)lane) * 4 + w] = 3u;
    }
#else
    // my wave's 1024 nodes inside a skipped block (SkipBlocks): no error, nothing to load, nothing anybody will read
    bool skippedN = skip_block(sk, brick, d, (chunk * 4u + (uint32_t)w) << 10);
    uint4 tvN = make_uint4(0, 0, 0, 0);
    uint2 pvN = make_uint2(0, 0);
    if (!skippedN) { const size_t i0 = ((size_t)chunk * 256u + threadIdx.x) * 16u; tvN = ld16(T + i0); pvN = ld8(P + (i0 >> 1)); }
    for (; chunk < chunkEnd; ++chunk) {
        const size_t i0 = ((size_t)chunk * 256u + threadIdx.x) * 16u;
        const bool skipped = skippedN;
        const uint4 tv = tvN;
        const uint2 pv = pvN;
        if (chunk + 1 < chunkEnd) {
            skippedN = skip_block(sk, brick, d, ((chunk + 1u) * 4u + (uint32_t)w) << 10);
            tvN = make_uint4(0, 0, 0, 0); pvN = make_uint2(0, 0);
            if (!skippedN) { const size_t i1 = i0 + 4096u; tvN = ld16(T + i1); pvN = ld8(P + (i1 >> 1)); }
        }
        uint32_t cpk, rw[4], s0, sm, sp;
        const bool busy = eval(tv, pv, skipped, cpk, rw, s0, sm, sp);
        if (sk.flag && d == sk.Dm2 && !busy && lane == 0) {      // (level D-2, see above)
            uint8_t *f = sk.flag + (int64_t)brick * sk.nBlk + (size_t)chunk * 4 + w;
            if (*f & 1u) *f = 3u;
        }
        if (!skipped && STORE) {
            st4(Cd + (i0 >> 2), cpk);
            st16(R + i0, make_uint4(rw[0], rw[1], rw[2], rw[3]));
        }
        if (lane == 0) {
            blockErr[(int64_t)brick * nErrBlk + (size_t)chunk * 4 + w] = s0;   // 1024 nodes per wave
            if (!STORE && needDF) {
                blockErr[errPlane + (int64_t)brick * nErrBlk + (size_t)chunk * 4 + w] = sm;
                blockErr[2 * errPlane + (int64_t)brick * nErrBlk + (size_t)chunk * 4 + w] = sp;
            }
        }
        accM += sm; accP += sp;
    }
#endif
    if ((threadIdx.x & 63) == 0) { shm[w] = accM; shp[w] = accP; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tm = shm[0] + shm[1] + shm[2] + shm[3], tp = shp[0] + shp[1] + shp[2] + shp[3];
        if (tm) atomicAdd(&c.errMinus, tm);
        if (tp) atomicAdd(&c.errPlus, tp);
    }
}

// End of epoch e and head of epoch e+1 of the while loop at R.cpp:275-366, one wave
// per brick.  `currentError += err^2` runs over the level in node order starting from
// a fractional carry (defect C-1), so the double rounds only when the running sum
// crosses a power of two: while the sum provably stays inside its binade every partial
// sum is exactly representable, so whole block partials (64 per step, prefix-summed
// across the wave) are added at once; the block in which the sum crosses is walked
// node by node with the reference's own rounded additions.
__device__ __forceinline__ double next_pow2_above(double s)
{
    int ex;
    frexp(s, &ex);              // s in [2^(ex-1), 2^ex)
    return ldexp(1.0, ex);
}

__device__ inline double ctl_walk_block(double s, const uint8_t *__restrict__ T, const uint8_t *__restrict__ P, int d,
                                        int dist, uint32_t lo, uint32_t hi, int lane)
{
    int tn = lo + lane < hi ? T[lo + lane] : 0, pn = (lo + lane < hi && d > 0) ? P[(lo + lane) >> 1] : 0;   // one step ahead
    for (uint32_t base = lo; base < hi; base += 64) {
        uint32_t i = base + lane;
        uint32_t e = 0;
        const int t = tn, p = pn;
        {
            const uint32_t i2 = i + 64;
            tn = i2 < hi ? T[i2] : 0;
            pn = (i2 < hi && d > 0) ? P[i2 >> 1] : 0;
        }
        if (i < hi) {
            int er = encode_node(t, p, dist).err;
            e = (uint32_t)(er * er);
        }
        const uint32_t incl = wave_incl_scan_u32(e, lane);
        const uint32_t total = lane_u32(incl, 63);
        uint32_t consumed = 0;
        int start = 0;
        while (true) {
            bool ok = true;
            if (lane >= start && s != 0.0) ok = (s + (double)(incl - consumed)) < next_pow2_above(s);
            const unsigned long long bad = ~__ballot(ok);
            if (bad == 0ull) { s = s + (double)(total - consumed); break; }
            const int f = __ffsll((long long)bad) - 1;
            const uint32_t exclF = lane_u32(incl - e, f), eF = lane_u32(e, f);
            s = s + (double)(exclF - consumed);   // exact: still inside the binade
            s = s + (double)eF;                   // the reference's rounded add that crosses it
            consumed = exclF + eF;
            start = f + 1;
        }
    }
    return s;
}

// The same walk for a whole 1024-node block with 16 consecutive nodes per lane: one load round trip, the err^2
// prefix sums built once (local prefix + one wave scan), and every crossing found by comparing each node's
// prefix with the current bound -- instead of sixteen dependent 64-node steps.
__device__ inline double ctl_walk_block16(double s, const uint8_t *__restrict__ T, const uint8_t *__restrict__ P, int dist,
                                          uint32_t lo, int lane)
{
    const uint4 tv = *(const uint4 *)(T + lo + lane * 16);
    const uint2 pv = *(const uint2 *)(P + (lo >> 1) + lane * 8);
    const uint32_t tw[4] = {tv.x, tv.y, tv.z, tv.w}, pw[2] = {pv.x, pv.y};
    const uint32_t d2 = (uint32_t)dist * 0x10001u;
    uint32_t e[16], pre[16];          // err^2 of my nodes, inclusive prefix inside the lane
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const EncPair c = enc_pair(tw[j >> 1], j & 1, pw[j >> 2], j & 3);
        const vr_s16x2 er = enc_pair_err(c, d2);
        e[2 * j] = (uint32_t)((int)er.x * (int)er.x);
        e[2 * j + 1] = (uint32_t)((int)er.y * (int)er.y);
        run += e[2 * j]; pre[2 * j] = run;
        run += e[2 * j + 1]; pre[2 * j + 1] = run;
    }
    const uint32_t inclL = wave_incl_scan_add_dpp(run);       // < 2^27
    const uint32_t baseL = inclL - run, total = (uint32_t)__builtin_amdgcn_readlane((int)inclL, 63);
    uint32_t consumed = 0;
    int startPos = 0;                                          // nodes before block-local position startPos are added
    while (true) {
        // first node at or after startPos whose addition (with everything before it) would leave the binade
        int fail = 16;
        if (s != 0.0) {
            const double bound = next_pow2_above(s);
#pragma unroll
            for (int k = 15; k >= 0; --k)
                if (lane * 16 + k >= startPos && !((s + (double)(baseL + pre[k] - consumed)) < bound)) fail = k;
        }
        const unsigned long long bad = __ballot(fail < 16);
        if (bad == 0ull) { s = s + (double)(total - consumed); break; }
        const int f = __ffsll((long long)bad) - 1;
        const int kF = __builtin_amdgcn_readlane(fail, f);
        uint32_t eF = 0, gF = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k == kF) { eF = e[k]; gF = baseL + pre[k]; }
        eF = (uint32_t)__builtin_amdgcn_readlane((int)eF, f);
        gF = (uint32_t)__builtin_amdgcn_readlane((int)gF, f);
        s = s + (double)(gF - eF - consumed);   // exact: still inside the binade
        s = s + (double)eF;                     // the reference's rounded add that crosses it
        consumed = gF;
        startPos = f * 16 + kF + 1;
    }
    return s;
}

// 64 partials (1024 nodes each) starting at block `base`, added in order: whole partials while the sum stays inside
// its binade, the crossing block node by node
#define CTL_STAGE_BLOCKS 8192       // k_control keeps a level's per-block partials in LDS when there are at most this many (32 KiB)
__device__ inline double ctl_partials64(double s, const unsigned long long *__restrict__ be, const uint32_t *stg, uint32_t base, uint32_t nblk,
                                        const uint8_t *__restrict__ T, const uint8_t *__restrict__ P, int d, int dist,
                                        uint32_t n, int lane)
{
    const unsigned long long e2 = base + lane < nblk ? (stg ? (unsigned long long)stg[base + lane] : be[base + lane]) : 0ull;
    // two 32-bit DPP scans (24-bit limbs: 64 partials of < 2^27 each cannot overflow either)
    const unsigned long long incl = (unsigned long long)wave_incl_scan_add_dpp((uint32_t)(e2 & 0xFFFFFFull)) +
                                    ((unsigned long long)wave_incl_scan_add_dpp((uint32_t)(e2 >> 24)) << 24);
    const unsigned long long total = lane_u64(incl, 63);
    unsigned long long consumed = 0;
    int start = 0;
    while (true) {
        bool ok = true;
        // an integer-valued sum below 2^53 adds integers exactly whatever the binade
        const bool sInt = (s == floor(s)) && (s + (double)(total - consumed)) < 9007199254740992.0;
        if (lane >= start && !sInt) ok = (s + (double)(incl - consumed)) < next_pow2_above(s);
        const unsigned long long bad = ~__ballot(ok);
        if (bad == 0ull) { s = s + (double)(total - consumed); break; }
        const int f = __ffsll((long long)bad) - 1;
        const unsigned long long exclF = lane_u64(incl - e2, f), inclF = lane_u64(incl, f);
        s = s + (double)(exclF - consumed);
        uint32_t lo = (base + f) * FILL_NODES_PER_BLOCK, hi = lo + FILL_NODES_PER_BLOCK;
        if (hi > n) hi = n;
        s = (hi - lo == 1024u && d > 0) ? ctl_walk_block16(s, T, P, dist, lo, lane) : ctl_walk_block(s, T, P, d, dist, lo, hi, lane);
        consumed = inclF;
        start = f + 1;
    }
    return s;
}

__global__ void __launch_bounds__(64)
k_control(int d, int maxEpochs, int guarded, Ctrl *ctrls, const uint8_t *__restrict__ temp, int64_t heapStride,
          ReconBufs rb, int64_t leafStride, const unsigned long long *__restrict__ blockErr, int64_t nErrBlk, int64_t errPlane,
          int leaflessLeaf)
{
    const int brick = blockIdx.x, lane = threadIdx.x;
    __shared__ __attribute__((aligned(16))) uint32_t ctlStage[CTL_STAGE_BLOCKS];
    Ctrl &c = ctrls[brick];
    if (c.constBrick) return;
    const uint32_t n = 1u << d;
    const bool ending = c.active && c.fillThisEpoch;
    double s = c.currentError;
    if (ending) {
        const uint8_t *T = temp + (int64_t)brick * heapStride + ((int64_t)1 << d);
        const uint8_t *P = rb.b[c.par] + (int64_t)brick * leafStride;
        const int dist = (int)(uint8_t)c.currentDistance;
        const uint32_t nblk = (n + FILL_NODES_PER_BLOCK - 1) / FILL_NODES_PER_BLOCK;
        const unsigned long long *be = blockErr + (int64_t)c.altSel * errPlane + (int64_t)brick * nErrBlk;
        // Two levels: every lane sums one chunk of 64 partials (64 independent loads, no dependent steps), the wave
        // adds whole chunks in order while the running double provably stays inside its binade, and only a chunk in
        // which it crosses a power of two is opened (ctl_partials64, which opens only the crossing block).  A level
        // has ~log2 crossings, so this touches a handful of chunks instead of stepping through all of them.
        const uint32_t nchunk = (nblk + 63u) >> 6;
        // the partials (each < 2^27) go to LDS in one batch of coalesced loads: the chunk sums and every chunk that is
        // opened below then cost no memory round trip (64 uncoalesced 8-byte loads per lane in dependent batches, and
        // one more round trip per opened chunk, were a third of this kernel's 25-75 us)
        const uint32_t *stg = nullptr;
        if (nblk >= 256u && nblk <= (uint32_t)CTL_STAGE_BLOCKS && (nblk & 255u) == 0u) {
            for (uint32_t i = (uint32_t)lane * 4u; i < nblk; i += 256u) {
                const uint4 a = *(const uint4 *)(be + i), b = *(const uint4 *)(be + i + 2);
                *(uint4 *)(ctlStage + i) = make_uint4(a.x, a.z, b.x, b.z);
            }
            stg = ctlStage;
        }
        for (uint32_t cb = 0; cb < nchunk; cb += 64) {
            const uint32_t ch = cb + (uint32_t)lane;
            unsigned long long tot = 0;
            if (ch < nchunk && stg) {
                const uint32_t *q = stg + (size_t)ch * 64;      // (whole chunks: nblk is a multiple of 256)
#pragma unroll 8
                for (int k = 0; k < 64; ++k) tot += q[(k + lane) & 63];      // rotated: the lanes' rows sit 64 words apart
            } else if (ch < nchunk) {
                const unsigned long long *q = be + (size_t)ch * 64;
                const uint32_t m = nblk - ch * 64 < 64u ? nblk - ch * 64 : 64u;
                if (m == 64u) {
#pragma unroll 8
                    for (int k = 0; k < 64; ++k) tot += q[k];
                } else
                    for (uint32_t k = 0; k < m; ++k) tot += q[k];
            }
            // chunk totals < 2^33: 24-bit low limbs (sum < 2^30) and high limbs < 2^9 (sum < 2^15)
            const unsigned long long incl = (unsigned long long)wave_incl_scan_add_dpp((uint32_t)(tot & 0xFFFFFFull)) +
                                            ((unsigned long long)wave_incl_scan_add_dpp((uint32_t)(tot >> 24)) << 24);
            const unsigned long long total = lane_u64(incl, 63);
            unsigned long long consumed = 0;
            int start = 0;
            while (true) {
                bool ok = true;
                const bool sInt = (s == floor(s)) && (s + (double)(total - consumed)) < 9007199254740992.0;
                if (lane >= start && !sInt) ok = (s + (double)(incl - consumed)) < next_pow2_above(s);
                const unsigned long long bad = ~__ballot(ok);
                if (bad == 0ull) { s = s + (double)(total - consumed); break; }
                const int f = __ffsll((long long)bad) - 1;
                const unsigned long long exclF = lane_u64(incl - tot, f), inclF = lane_u64(incl, f);
                s = s + (double)(exclF - consumed);       // exact: still inside the binade
                s = ctl_partials64(s, be, stg, (cb + (uint32_t)f) * 64u, nblk, T, P, d, dist, n, lane);
                consumed = inclF;
                start = f + 1;
            }
        }
    }
    if (lane != 0) return;
    if (ending) {
        c.roleDist[c.cur] = (int)(uint8_t)c.currentDistance;   // what this epoch's fill wrote its buffer and the codes with
        c.codesDist = (int)(uint8_t)c.currentDistance;
        // (a real fill that made the central difference leaves its minus / plus partials behind)
        c.altValid = leaflessLeaf && !c.altSel && c.epoch + 1 < maxEpochs;
        c.altDist = (int)(uint8_t)c.currentDistance;
        c.altSel = 0;
        c.currentError = s / (double)n;                        // R.cpp:315
        if (c.currentError < 1.0) {                            // R.cpp:319
            c.active = 0;
        } else if (c.epoch != 0 && c.currentError > c.previousError) { // revert R.cpp:323-331
            c.currentError = c.previousError;
            c.currentDistance = c.previousDistance;
            c.currentDF = c.previousDF;
            c.currentStepSize = c.previousStepSize / 2.0;
            int tmp = c.cur; c.cur = c.prev; c.prev = tmp;     // recon.swap(reconPreviousEpoch)
            c.pendingEqual = 0;
            c.numReverts++;
            c.epoch++;
        } else {
            if (!guarded || c.epoch + 1 < maxEpochs) {         // VolumeKdtree.cpp:333 guard
                double e0 = (double)c.errMinus / (double)n;    // R.cpp:346,357
                double e1 = (double)c.errPlus / (double)n;
                c.currentDF = (e1 - e0) / 2.0;                 // R.cpp:361, h = 1
                c.currentStepSize = fmax(-4.0, fmin(4.0, -1.25 * c.currentDF));
                // reconPreviousEpoch = recon (R.cpp:364) without a copy: the buffer just
                // written becomes the snapshot and the next fill goes to the other one.
                c.prev = c.cur;
                c.cur = 1 - c.cur;
                c.pendingEqual = 1;
            }
            c.epoch++;
        }
    }
    if (c.active) {                                            // while-condition + loop head
        if (!(c.epoch < maxEpochs && fabs(c.previousStepSize) >= 0.5)) {
            c.active = 0;
        } else if (c.epoch != 0) {
            c.previousDistance = c.currentDistance;
            c.previousError = c.currentError;
            c.previousDF = c.currentDF;
            c.previousStepSize = c.currentStepSize;
            c.currentDistance = round(fmin(255.0, fmax(0.0, c.previousDistance + c.previousStepSize)));
            if (c.currentDistance == c.previousDistance) c.active = 0; // R.cpp:287-288
        }
    }
    c.fillThisEpoch = c.active;
    c.errMinus = c.errPlus = 0;
    if (c.active) c.pendingEqual = 0; // the coming fill overwrites the non-snapshot buffer
    // the coming epoch is the last that can run (no central difference of its own) and sits one step beside the fill
    // whose partials are in memory: no fill
    if (leaflessLeaf && c.active && c.altValid && c.epoch + 1 >= maxEpochs) {
        const int nd = (int)(uint8_t)c.currentDistance;
        const int dm = (int)(uint8_t)fmax(0.0, (double)c.altDist - 1.0), dp = (int)(uint8_t)fmin(255.0, (double)c.altDist + 1.0);   // k_fill16's distM / distP
        if (nd != c.altDist) c.altSel = nd == dm ? 1 : (nd == dp ? 2 : 0);
    }
}

// R.cpp:369-381: record the level's distance, make its reconstruction the next level's parents.
__global__ void k_level_end(int d, Ctrl *ctrls)
{
    if (threadIdx.x) return;
    Ctrl &c = ctrls[blockIdx.x];
    if (c.constBrick) return;
    c.distanceMap[d] = (uint8_t)c.currentDistance;
    int finalRole = c.pendingEqual ? c.prev : c.cur;
    c.finalReconDist = c.roleDist[finalRole];
    c.finalCodesDist = c.codesDist;
    int finalPhys = phys_buf(c, finalRole);
    int otherPhys = phys_buf(c, 1 - finalRole);
    int oldPar = c.par;
    c.par = finalPhys;
    c.ra = oldPar;
    c.rb = otherPhys;
    c.cur = 0; c.prev = 1; c.pendingEqual = 0;
    c.active = 0; c.fillThisEpoch = 0;
    c.altValid = 0; c.altSel = 0;
}

// Levels D-1 and D of the constant 4096-leaf blocks that the level loop will visit: k_pyramid12 left them unwritten
// (SkipBlocks builds).  Between the end of level D-2 and the head of level D-1, when bit 1 of the flags is final: a
// block with bit 0 set and bit 1 clear, in a brick that is not constant, gets 4096 + 2048 bytes of its own
// depth-(D-12) truth (the voxel value in the mid stream, 0 in the half-range stream).  A wave takes 64 consecutive
// blocks at a time, one flag and one root byte per lane, and writes the blocks that need it one after the other
// (6 KiB each, six 16-byte streaming stores per lane).
__global__ void __launch_bounds__(256)
k_fill_const_leaves(int D, const Ctrl *ctrls, uint8_t *__restrict__ temp, int64_t heapStride, SkipBlocks sk)
{
    const int brick = blockIdx.y, lane = threadIdx.x & 63;
    if (ctrls[brick].constBrick) return;
    uint8_t *T = temp + (int64_t)brick * heapStride;
    const uint8_t *flag = sk.flag + (int64_t)brick * sk.nBlk;
    const uint32_t nBlk = (uint32_t)sk.nBlk;
    for (uint32_t b0 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; b0 < nBlk; b0 += gridDim.x * 256u) {
        const uint32_t blk = b0 + (uint32_t)lane;
        uint32_t v = 0;
        bool need = false;
        if (blk < nBlk) {
            need = (flag[blk] & 3u) == 1u;
            v = T[((int64_t)1 << (D - 12)) + blk];
        }
        unsigned long long todo = __ballot(need);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)v, l) * 0x01010101u;
            const uint4 wv = make_uint4(w, w, w, w);
            uint8_t *leafL = T + ((int64_t)1 << D) + ((int64_t)(b0 + (uint32_t)l) << 12) + lane * 16;
            uint8_t *parL = T + ((int64_t)1 << (D - 1)) + ((int64_t)(b0 + (uint32_t)l) << 11) + lane * 16;
#pragma unroll
            for (int j = 0; j < 4; ++j) st16(leafL + j * 1024, wv);
#pragma unroll
            for (int j = 0; j < 2; ++j) st16(parL + j * 1024, wv);
        }
    }
}

// The range stream's prune follows the mid stream (M.cpp:864-865); see k_prune_*.
// ------------------------------------------------------------------ prune ----
// per-block statistics record: sum |recon - truth| after growth (40 bits) | max error before << 40 | max after << 48
__device__ __forceinline__ unsigned long long stat_pack(unsigned long long l1, int maxBefore, int maxAfter)
{
    return l1 | ((unsigned long long)maxBefore << 40) | ((unsigned long long)maxAfter << 48);
}
__device__ __forceinline__ unsigned long long stat_merge(unsigned long long a, unsigned long long b)
{
    const unsigned long long M40 = (1ull << 40) - 1ull;
    const unsigned long long mb = max((a >> 40) & 255ull, (b >> 40) & 255ull), ma = max((a >> 48) & 255ull, (b >> 48) & 255ull);
    return ((a & M40) + (b & M40)) | (mb << 40) | (ma << 48);
}
__global__ void __launch_bounds__(256)
k_prune_leaf(int D, int tol, Ctrl *ctrls, const uint8_t *__restrict__ temp, uint8_t *__restrict__ codes,
             uint8_t *__restrict__ codesRange, int64_t heapStride, int64_t codeStride, ReconBufs rb, int64_t leafStride,
             int maxDepth,
             unsigned long long *__restrict__ blockL1, int64_t nEmitBlk)
{
    __shared__ unsigned long long shl[4];
    const int brick = blockIdx.y;
    Ctrl &c = ctrls[brick];
    if (c.constBrick) return;
    const uint32_t n = 1u << D;
    uint32_t r = blockIdx.x * 256u + threadIdx.x;
    int err = 0, fe = 0;
    if (r < n) {
        const int64_t hi = (int64_t)brick * heapStride + ((int64_t)1 << D) + r;
        int t = temp[hi];
        int rec = rb.b[c.par][(int64_t)brick * leafStride + r];
        err = rec > t ? rec - t : t - rec;
        fe = err;
        uint8_t *Cb = codes + (int64_t)brick * codeStride;
        const int64_t ci = ((int64_t)1 << D) + r;
        const int code = cget(Cb, ci);
        if (code == 0 && err < tol) {        // R.cpp:618-626 (leaf: no children)
            cset3(Cb, ci);
            if (codesRange) cset3(codesRange + (int64_t)brick * codeStride, ci);
        } else if (code != 3) {              // an unpruned leaf is always live: its error after branch growth
            int depth = D;
            while (depth < maxDepth) {
                const int e2 = rec > t ? rec - t : t - rec;
                if (e2 > tol) { ++depth; rec = encode_node(t, rec, 64 >> (depth - D - 1)).recon; }
                else break;
            }
            fe = rec > t ? rec - t : t - rec;
        }
    }
    int fm = fe;
    unsigned long long l1 = (unsigned long long)fe;
    for (int o = 32; o > 0; o >>= 1) {
        int u = __shfl_xor(err, o); err = u > err ? u : err;
        int w = __shfl_xor(fm, o); fm = w > fm ? w : fm;
        l1 += __shfl_xor(l1, o);
    }
    // statistics leave as per-block records (no atomics on the brick's control block: every wave of a
    // brick hitting one address serialises on one L2 channel); k_emit_stats reduces them
    if ((threadIdx.x & 63) == 0) shl[threadIdx.x >> 6] = stat_pack(l1, err, fm);    // R.cpp:71-76, 115-129
    __syncthreads();
    if (threadIdx.x == 0)
        blockL1[(int64_t)brick * nEmitBlk + blockIdx.x] = stat_merge(stat_merge(shl[0], shl[1]), stat_merge(shl[2], shl[3]));
}

__global__ void __launch_bounds__(256)
k_prune_level(int d, const Ctrl *ctrls, uint8_t *__restrict__ codes, uint8_t *__restrict__ codesRange, int64_t codeStride)
{
    const int brick = blockIdx.y;
    if (ctrls[brick].constBrick) return;
    const uint32_t n = 1u << d;
    uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    uint8_t *Cb = codes + (int64_t)brick * codeStride;
    const int64_t me = ((int64_t)1 << d) + p, ch = ((int64_t)1 << (d + 1)) + 2 * (int64_t)p;
    if (cget(Cb, ch) == 3 && cget(Cb, ch + 1) == 3 && cget(Cb, me) == 0) {  // R.cpp:624
        cset3(Cb, me);
        if (codesRange) cset3(codesRange + (int64_t)brick * codeStride, me);
    }
}

// The grown branch of a leaf (R.cpp:655-704: encodeNode against the leaf's own reconstruction with
// distances 64, 32, .., 1 until the error is within tolerance) depends only on the initial error
// m0 = |truth - recon| and the side, as long as the clamps at 0 / 255 cannot matter: a clamped step
// lands min(truth, 255 - truth) away from the truth, which is never an improvement while that is
// >= the current error.  lut[m0] = final error | count << 8 | tokens << 16 (2 bits each, "add" = towards the truth
// first; byte-aligned so that two entries fold into packed lanes with one v_perm each); the other side swaps
// add <-> sub.  Leaves with m0 > min(t, 255 - t) take
// the exact step-by-step path.
#define VR_CHAIN_LUT_SIGNED 260     // word offset of the signed-key table inside BrickSet::chainLut (512 entries)
__global__ void k_chain_lut(int tol, int nsteps, uint32_t *__restrict__ lut)
{
    const int m0 = threadIdx.x, t = 128;
    int rec = m0 <= 127 ? t - m0 : 0;
    uint32_t bits = 0, n = 0;
    int lastKeep = 0;                 // the last evaluated branch node kept its parent's value (code 0)
    for (int i = 0; i < nsteps; ++i) {
        const int err = rec > t ? rec - t : t - rec;
        if (err > tol) { const Enc e = encode_node(t, rec, 64 >> i); rec = e.recon; bits |= (uint32_t)e.code << (2 * n); ++n; lastKeep = e.code == 0; }
        else { bits |= 3u << (2 * n); ++n; break; }
    }
    const int fe = rec > t ? rec - t : t - rec;
    lut[m0] = (uint32_t)fe | (n << 8) | (bits << 16);     // byte 0: final error, byte 1: token count, bytes 2-3: tokens
    // the same keyed by the SIGNED error truth - reconstruction (9 bits, at lut + VR_CHAIN_LUT_SIGNED): a negative error
    // takes the mirrored branch (add <-> sub), so k_prune_emit12 needs neither the mirror nor the select
    lut[VR_CHAIN_LUT_SIGNED + m0] = lut[m0];
    if (m0 >= 1) lut[VR_CHAIN_LUT_SIGNED + 512 - m0] = (uint32_t)fe | (n << 8) | ((bits ^ (((bits ^ (bits >> 1)) & 0x1555u) * 3u)) << 16);
    if (m0 == 0) lut[VR_CHAIN_LUT_SIGNED + 256] = 0;
    // entries 0..127 are the ones a leaf can reach through the table (m0 <= min(t, 255 - t)); one that ends on a
    // "keep" would need the reference's zero-run rewrite (R.cpp:662-669,686-688): counted, asserted zero by the tests
    const int zr = __syncthreads_count(m0 <= 127 && lastKeep);
    if (m0 == 0) lut[256] = (uint32_t)zr;
}

// ---------------------------------------------------------------- convert ----
// Tokens owned by leaf rank r, in stream order: the live internal nodes whose first
// leaf is r (depth ascending), then the leaf token and its grown chain (R.cpp:655-704).
// A node is live iff it is the root or its parent was not pruned (pruning is closed
// downwards, so "some ancestor pruned" == "parent pruned").
struct Owned {
    unsigned long long spineBits; // 2 bits per token, first token in the low bits
    uint32_t leafBits;
    unsigned long long spineBitsR; // MidRangeTree: the range stream's codes for the same tokens
    uint32_t leafBitsR;
    int nSpine, nLeaf;
    int preDs;       // tokens owned by r that precede the depth-Ds node (index entry)
    int aliveAtDs;
    int finalErr;    // |recon - temp| of the leaf after branch growth (-1: leaf not visited)
    int zeroRun;     // the branch ended on an evaluated "keep" at the last level (Ctrl::zeroRun)
};

__device__ inline Owned owned_tokens(const uint8_t *__restrict__ Cb, const uint8_t *__restrict__ CbR,
                                     const uint8_t *__restrict__ Tb, const uint8_t *__restrict__ TbR,
                                     const uint8_t *__restrict__ Rl, const uint8_t *__restrict__ RlR, int D,
                                     int maxDepth, int tol, const uint8_t *dmap, const uint8_t *dmapR, int Ds,
                                     uint32_t r)
{
    Owned o;
    o.spineBits = 0; o.leafBits = 0; o.spineBitsR = 0; o.leafBitsR = 0;
    o.nSpine = 0; o.nLeaf = 0; o.preDs = 0; o.aliveAtDs = 0; o.finalErr = -1; o.zeroRun = 0;
    const int jmin = r ? D - (__ffs((int)r) - 1) : 0;
    bool alive = true;
    if (jmin > 0) alive = cget(Cb, ((int64_t)1 << (jmin - 1)) + (r >> (D - jmin + 1))) != 3;
    int j = jmin;
    for (; alive && j < D; ++j) {
        if (j == Ds) { o.preDs = o.nSpine; o.aliveAtDs = 1; }
        const int64_t ni = ((int64_t)1 << j) + (r >> (D - j));
        int code = cget(Cb, ni);
        o.spineBits |= (unsigned long long)code << (2 * o.nSpine);
        if (CbR) o.spineBitsR |= (unsigned long long)cget(CbR, ni) << (2 * o.nSpine);
        o.nSpine++;
        if (code == 3) alive = false;
    }
    if (alive) {
        if (Ds == D) { o.preDs = o.nSpine; o.aliveAtDs = 1; }
        const int64_t li = ((int64_t)1 << D) + r;
        int code = cget(Cb, li);
        o.leafBits = (uint32_t)code;
        if (CbR) o.leafBitsR = (uint32_t)cget(CbR, li);
        o.nLeaf = 1;
        int t = Tb[li], rec = Rl[r];
        int tR = 0, recR = 0;
        if (CbR) { tR = TbR[li]; recR = RlR[r]; }
        if (code != 3) {
            int depth = D;
            while (depth < maxDepth) {
                int err = rec > t ? rec - t : t - rec;
                if (err > tol) {                       // grow the branch (R.cpp:695-697, 657-660)
                    depth++;
                    Enc e = encode_node(t, rec, dmap[depth]);
                    rec = e.recon;
                    if (depth == maxDepth && e.code == 0) o.zeroRun = 1;
                    o.leafBits |= (uint32_t)e.code << (2 * o.nLeaf);
                    if (CbR) {                         // M.cpp: range stream re-encoded in lock-step
                        Enc er = encode_node(tR, recR, dmapR[depth]);
                        recR = er.recon;
                        o.leafBitsR |= (uint32_t)er.code << (2 * o.nLeaf);
                    }
                    o.nLeaf++;
                } else {                               // terminator (R.cpp:699-703, 671-674)
                    o.leafBits |= 3u << (2 * o.nLeaf);
                    if (CbR) o.leafBitsR |= 3u << (2 * o.nLeaf);
                    o.nLeaf++;
                    break;
                }
            }
        }
        o.finalErr = rec > t ? rec - t : t - rec;
    }
    return o;
}

struct EmitArgs {
    const uint8_t *codes, *codesR, *temp, *tempR;
    ReconBufs rb, rbR;
    Ctrl *ctrls, *ctrlsR;
    int64_t heapStride, leafStride, codeStride;
    int D, maxDepth, tol, Ds, K;
    uint32_t *blockTot, *blockOff;
    unsigned long long *blockOff64; // trees of more than 2^32 tokens (origTreeDepth > 28): the scan in 64 bits; index entries then
    unsigned long long *idxBase;    // stay relative to their 4096-leaf block and idxBase[block] holds the block's stream offset
    unsigned long long *blockL1;   // per-block sum |recon - temp| after growth (reduced by k_emit_stats)
    uint8_t *blockAlive, *blockVal; // k_block_alive: flags, scalar above the block
    unsigned long long *blockSpine; // k_block_alive: tokens above depth D-12 owned by the block's first rank
    unsigned long long *blockSpineR; // ... the same tokens of MidRangeTree's range stream
    int64_t nEmitBlk;
    uint8_t *tree, *treeR;
    int64_t treeCap;
    const unsigned long long *brickOff;   // compact_launch: brick b's stream starts at tree + brickOff[b] (else at tree + b * treeCap)
    int64_t compactCap;
    uint32_t *idxOff;
    uint8_t *idxVal;
    uint8_t *idxVal3;              // k_concat12: decoded scalars of the depth-(D-3) nodes (k_decode_quad)
    int64_t nIdx;
    const uint32_t *chainLut;
};

__device__ inline uint32_t block_excl_scan_u32(uint32_t v, uint32_t *shWave, uint32_t &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan_add_dpp(v);
    if (lane == 63) shWave[w] = incl;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) { if (i < w) woff += shWave[i]; tot += shWave[i]; }
    __syncthreads();
    total = tot;
    return woff + incl - v;
}

// the same for a block of exactly four waves: four LDS reads, no loop over a run-time wave count
__device__ __forceinline__ uint32_t block4_excl_scan_u32(uint32_t v, uint32_t *shWave, uint32_t &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan_add_dpp(v);
    if (lane == 63) shWave[w] = incl;
    __syncthreads();
    const uint32_t s0 = shWave[0], s1 = shWave[1], s2 = shWave[2], s3 = shWave[3];
    __syncthreads();
    total = s0 + s1 + s2 + s3;
    const uint32_t woff = w == 0 ? 0u : (w == 1 ? s0 : (w == 2 ? s0 + s1 : s0 + s1 + s2));
    return woff + incl - v;
}

// 1: k_prune_emit12 prunes depths D-5 .. D-12 by wave 0 in registers, behind one batch of LDS reads and in front of one
// workgroup barrier, while waves 1 .. 3 clear the string buffer.  0: the code as it was -- an eight-level LDS loop with
// a barrier per level that all four waves run -- for a trace of the old behaviour.
#ifndef VR_PRUNE_CHAIN
#define VR_PRUNE_CHAIN 1
#endif

// ---- prune + block-local emit (VolumeKdtree streams with D >= 12: K = 6, Ds = D-6) --------------
// One block owns a depth-(D-12) subtree: 4096 leaves, 16 per thread.  It prunes the twelve levels
// bottom-up (the four above the leaves in registers, the other eight in LDS), and then,
// top-down, writes the subtree's own preorder token string -- assuming its root is live -- into LDS
// and from there into the block's slot of the brick's stream buffer: slot b starts at word b * PE_WORDS
// (a block's string is at most 4095 + 8 * 4096 tokens = 9216 bytes).  That block-gapped buffer IS what the decoders
// read (k_index12 points the decode index at the slots); the reference's contiguous layout (R.cpp:631-724 writes one
// array) is produced from it by k_concat12 when somebody asks for the bytes -- vr_brickset_get_tree, save,
// get_packed4 -- not on the build -> levelCut path, where that copy was 4.5 ms of a 43 ms build.
#define PE_WORDS 2320
#define PE_TOKENS (PE_WORDS * 16)

struct PruneEmitArgs {
    int D, tol, maxDepth;
    Ctrl *ctrls;
    uint8_t *temp;                 // truths (leaf half, read) / staging (internal half, written)
    uint8_t *codes;
    int64_t heapStride, codeStride, leafStride;
    ReconBufs rb;
    uint32_t *subTok;              // tokens of the block's subtree (k_block_alive reads it from blockOff[])
    int64_t nEmitBlk;
    unsigned long long *blockL1;
    const uint32_t *chainLut;
    uint32_t *idxOff;              // block-local token offset of every depth-Ds node (k_concat12 makes it global)
    int64_t nIdx;
    uint32_t *fineIdx;             // 16 bytes per depth-Ds node: tokens owned by each of its 4-leaf subtrees (k_decode_fine)
    // MidRangeTree's second stream (k_prune_emit12<true>): its own truths, codes, reconstruction, control blocks
    Ctrl *ctrlsR;
    uint8_t *tempR, *codesR;
    ReconBufs rbR;
    uint8_t *gap, *gapR;           // the streams' block-gapped buffers (Stream2::tree)
    int64_t treeCap;
    SkipBlocks sk, skR;            // blocks the level loop left alone below depth D-2: all "keep", exactly reproduced (per stream)
    int uniformBlocks;             // constant blocks (flag bit 0) are k_prune_emit12_const's: k_prune_emit12<false, true> leaves them alone
    uint32_t *boxUniform;          // BrickSet::boxUniform: zero when the prune starts; k_prune_emit12_const sets the boxes it composes a string for
};

__device__ __forceinline__ void pe_put(uint32_t *W, uint32_t bitpos, unsigned long long v, int ntok)
{   // v: at most 44 bits of tokens
    if (ntok <= 0) return;
    const uint32_t sh = bitpos & 31u, w = bitpos >> 5;
    const unsigned long long lo = v << sh;
    atomicOr(&W[w], (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) atomicOr(&W[w + 1], (uint32_t)(lo >> 32));
    const uint32_t hi = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
    if (hi) atomicOr(&W[w + 2], hi);
}

// The leaf stage of k_prune_emit12 for one sibling pair in packed 16-bit lanes (k_prune_emit12_const evaluates one pair
// per constant block with the same code).  dl: truth minus reconstruction, cl2: the pair's level-loop codes.  Prune
// (R.cpp:618-626), then the grown branch from the table (k_chain_lut) where no clamp can matter; the lanes in `act`
// are left to pe_leaf_step.  bothMask gets bit 2j where both leaves are pruned tokens.
template <class LUT>     // lut(k): entry k of k_chain_lut's signed-key table, wherever the caller keeps it
__device__ __forceinline__ void pe_leaf_table(uint32_t T2, vr_s16x2 dl, uint32_t cl2, uint32_t tol2, const LUT &lut, vr_s16x2 &mxB,
                                                  uint32_t &m, uint32_t &sg, uint32_t &act, uint32_t &Lb, uint32_t &nt,
                                                  uint32_t &bothMask, int j)
{
    const vr_s16x2 mm = pk_abs(dl);
    m = pk_u(mm);
    sg = pk_u(dl >> 15);
    mxB = __builtin_elementwise_max(mxB, mm);
    const uint32_t lt = pk_u((mm - pk_s(tol2)) >> 15);                                     // err < tol
    const uint32_t isz = pk_u((pk_s(cl2) - pk_s(0x00010001u)) >> 15), is3 = pk_u((pk_s(0x00020002u) - pk_s(cl2)) >> 15);
    const uint32_t newp = isz & lt;
    const uint32_t pruned = newp | is3;
    const uint32_t lcode = cl2 | (newp & 0x00030003u);
    bothMask |= ((pruned & (pruned >> 16)) & 1u) << (2 * j);     // at the bit of the pair node's code (k_prune_emit12's upper levels)
    const vr_s16x2 lim = __builtin_elementwise_min(pk_s(T2), pk_s(T2 ^ 0x00FF00FFu));
    const uint32_t viol = pk_u((lim - mm) >> 15);                                          // a clamp could matter
    const uint32_t e0 = lut(pk_u(dl) & 511u), e1 = lut((pk_u(dl) >> 16) & 511u);           // keyed by the signed error
    const uint32_t useL = ~pruned & ~viol;
    const uint32_t ch2 = __builtin_amdgcn_perm(e1, e0, 0x07060302u);                           // the two token strings
    Lb = lcode | ((useL & ch2) << 2);
    nt = 0x00010001u + (useL & __builtin_amdgcn_perm(e1, e0, 0x0c050c01u));            // the two counts
    m = (useL & __builtin_amdgcn_perm(e1, e0, 0x0c040c00u)) | (~useL & m);         // the two final errors
    act = ~pruned & viol;
}
// ... and step i (distance d2 = (64 >> i) in both lanes) of the exact path for the lanes in `act`, the leaves the table does not cover
__device__ __forceinline__ void pe_leaf_step(int i, int nsteps, uint32_t d2, uint32_t tol2, uint32_t T2, uint32_t &m, uint32_t &sg, uint32_t &act,
                                             uint32_t &Lb, uint32_t &nt, uint32_t &keepEnd, uint32_t &anyAct)
{
    const vr_s16x2 mm = pk_s(m);
    const uint32_t gt = pk_u((pk_s(tol2) - mm) >> 15);
    nt = pk_u(pk_s(nt) - pk_s(act));
    const uint32_t go = act & gt;
    const uint32_t term = (act ^ go) & 0x00030003u;                                 // R.cpp:699-703
    const uint32_t lim = (sg & T2) | (~sg & (T2 ^ 0x00FF00FFu));
    const vr_s16x2 x = __builtin_elementwise_min(pk_s(d2) - mm, pk_s(lim));
    const vr_s16x2 nx = (vr_s16x2)(0) - x, ax = __builtin_elementwise_max(x, nx);
    const uint32_t take = go & pk_u((ax - mm) >> 15);
    const uint32_t dir = pk_u(pk_s(0x00010001u) - pk_s(sg));                        // add = 1, sub = 2
    Lb |= ((take & dir) | term) << (2 * i + 2);
    // an evaluated node that keeps leaves its error (> tol) unchanged, so the branch goes on unless this
    // was the last level: only there can a branch end on a "keep" (zero-run rewrite, see Ctrl::zeroRun)
    if (i == nsteps - 1) keepEnd |= go & ~take;
    m = (take & pk_u(ax)) | (~take & m);
    sg ^= take & pk_u(nx >> 15);
    act = go;
    anyAct |= go;
}

// RANGE (MidRangeTree, M.cpp:864-865, 871-982): the half-range stream has the mid stream's STRUCTURE -- a node is
// pruned, a branch grows and ends exactly where the mid stream's does -- and its own token VALUES: its level-loop codes,
// and along a branch encodeNode against its own reconstruction (M.cpp:930-933).  The second launch recomputes the mid
// stream's prune decisions and branch lengths from the mid arrays (same code, so the same result), swaps the range
// stream's values in, and writes the same string shape into the range stream's staging area.  Index, counts and
// statistics belong to the first launch.
template <bool RANGE, bool LEAFLESS>
__global__ void __launch_bounds__(256, RANGE ? 4 : 6)
k_prune_emit12(PruneEmitArgs a)
{
    __shared__ uint32_t lutS[512];                   // grown branch by signed initial error (k_chain_lut)
#if VR_PRUNE_CHAIN
    __shared__ __attribute__((aligned(16))) uint32_t W[PE_WORDS];
    __shared__ __attribute__((aligned(4))) uint8_t codeH[256], codeOldH[256];    // the block's nodes of depths D-12 .. D-5, heap order (1 .. 255)
    __shared__ __attribute__((aligned(4))) uint8_t fl4H[256];                    // "subtree is a single pruned token" flags of the depth-(D-4) nodes
    __shared__ __attribute__((aligned(8))) uint16_t cnt4H[256];                  // tokens their subtrees emit when live
#else
    __shared__ uint32_t W[PE_WORDS];
    __shared__ uint8_t codeH[256], codeOldH[256];    // the block's nodes of depths D-12 .. D-5, heap order (1 .. 255)
    __shared__ uint8_t flH[512];                     // "subtree is a single pruned token" flags; 256 + t = the depth-(D-4) nodes
    __shared__ uint16_t cntH[512];                   // tokens a live subtree emits
#endif
    __shared__ uint32_t shw[4];
    const int brick = blockIdx.y, t = threadIdx.x, D = a.D, tol = a.tol;
    Ctrl &c = a.ctrls[brick];
    const int cConst = c.constBrick, cPar = c.par, cRa = c.ra, cDistR = c.finalReconDist, cDistC = c.finalCodesDist;     // one scalar round trip
    if (cConst) return;
    const uint32_t blk = blockIdx.x, base = blk << 12;
    uint8_t *Cb = a.codes + (int64_t)brick * a.codeStride;
    uint32_t bflag = 0;
    if (!RANGE && LEAFLESS && a.uniformBlocks) {     // a constant block has a kernel of its own (k_prune_emit12_const)
        bflag = a.sk.flag[(int64_t)brick * a.sk.nBlk + blk];
        if (bflag & 1u) return;
    }
    // ---- every global load of the block, in one batch
    const uint32_t lutV = a.chainLut[VR_CHAIN_LUT_SIGNED + t], lutV2 = a.chainLut[VR_CHAIN_LUT_SIGNED + 256 + t];
    const int hU = t ? t : 1, lqU = 31 - __clz(hU);
    const int64_t niU = ((int64_t)1 << (D - 12 + lqU)) + ((int64_t)blk << lqU) + (hU - (1 << lqU));
    const uint32_t upB = Cb[niU >> 2];
    const int64_t n4 = ((int64_t)1 << (D - 4)) + (base >> 4) + t, n3 = ((int64_t)1 << (D - 3)) + (base >> 3) + 2 * t;
    const int64_t n2 = ((int64_t)1 << (D - 2)) + (base >> 2) + 4 * t, n1 = ((int64_t)1 << (D - 1)) + (base >> 1) + 8 * t;
    const uint32_t c4B = Cb[n4 >> 2], c3B = Cb[n3 >> 2], c2B = Cb[n2 >> 2];
    const int64_t li = ((int64_t)1 << D) + base + t * 16;
    // a block the level loop skipped (SkipBlocks) has no codes and no reconstruction in memory at depths D-1 and D:
    // they are all "keep" and exact, which is what zeros here say
    const bool skipB = (!RANGE && LEAFLESS && a.uniformBlocks) ? (bflag & 2u) != 0u
                                                                : a.sk.flag && (a.sk.flag[(int64_t)brick * a.sk.nBlk + blk] & 2u) != 0u;
    uint32_t c1H = 0, cpk = 0;
    uint4 tv = make_uint4(0, 0, 0, 0), rv = make_uint4(0, 0, 0, 0);
    uint2 pv = make_uint2(0, 0), pvR = make_uint2(0, 0);      // leafless: my leaves' eight parents (the level loop's last parents buffer but one)
    if (!skipB) {
        c1H = *(const uint16_t *)(Cb + (n1 >> 2));
        tv = *(const uint4 *)(a.temp + (int64_t)brick * a.heapStride + li);
        if (LEAFLESS)
            pv = *(const uint2 *)((cRa == 0 ? a.rb.b[0] : (cRa == 1 ? a.rb.b[1] : a.rb.b[2])) + (int64_t)brick * a.leafStride + (base >> 1) + t * 8);
        else {
            cpk = *(const uint32_t *)(Cb + (li >> 2));       // my 16 leaf codes, packed
            rv = *(const uint4 *)((cPar == 0 ? a.rb.b[0] : (cPar == 1 ? a.rb.b[1] : a.rb.b[2])) + (int64_t)brick * a.leafStride + base + t * 16);
        }
    }
    // RANGE: the same pieces of the range stream
    uint8_t *CbR = RANGE ? a.codesR + (int64_t)brick * a.codeStride : nullptr;
    uint32_t upBR = 0, c4BR = 0, c3BR = 0, c2BR = 0, c1HR = 0, cpkR = 0;
    uint4 tvR = make_uint4(0, 0, 0, 0), rvR = make_uint4(0, 0, 0, 0);
    int cDistRR = 0, cDistCR = 0;
    bool skipBR = false;
    if (RANGE) {
        const Ctrl &cr = a.ctrlsR[brick];
        const int cParR = cr.par, cRaR = cr.ra;
        cDistRR = cr.finalReconDist; cDistCR = cr.finalCodesDist;
        upBR = CbR[niU >> 2]; c4BR = CbR[n4 >> 2]; c3BR = CbR[n3 >> 2]; c2BR = CbR[n2 >> 2];
        // (a block the range stream's level loop skipped: all "keep" and exact there, like the mid stream's above)
        skipBR = a.skR.flag && (a.skR.flag[(int64_t)brick * a.skR.nBlk + blk] & 2u) != 0u;
        if (!skipBR) {
            c1HR = *(const uint16_t *)(CbR + (n1 >> 2));
            tvR = *(const uint4 *)(a.tempR + (int64_t)brick * a.heapStride + li);
            if (LEAFLESS)
                pvR = *(const uint2 *)((cRaR == 0 ? a.rbR.b[0] : (cRaR == 1 ? a.rbR.b[1] : a.rbR.b[2])) + (int64_t)brick * a.leafStride + (base >> 1) + t * 8);
            else {
                cpkR = *(const uint32_t *)(CbR + (li >> 2));
                rvR = *(const uint4 *)((cParR == 0 ? a.rbR.b[0] : (cParR == 1 ? a.rbR.b[1] : a.rbR.b[2])) + (int64_t)brick * a.leafStride + base + t * 16);
            }
        }
    }
    // leafless: the leaf stage below encodes every sibling pair itself; all that is needed up here is "every truth equals
    // its parent's reconstruction" (then all codes are "keep" and the leaves exact: what cpk == 0, tv == rv say)
    if (LEAFLESS) {
        rv = tv;
        cpk = ((tv.x ^ __builtin_amdgcn_perm(0, pv.x, 0x01010000u)) | (tv.y ^ __builtin_amdgcn_perm(0, pv.x, 0x03030202u)) |
               (tv.z ^ __builtin_amdgcn_perm(0, pv.y, 0x01010000u)) | (tv.w ^ __builtin_amdgcn_perm(0, pv.y, 0x03030202u))) != 0u ? 1u : 0u;
    }
    lutS[t] = lutV; lutS[256 + t] = lutV2;
    // ---- a block of 4096 exactly reproduced leaves under all-"keep" codes (constant regions) is one pruned subtree:
    // its string is the single token 3, its index entries are "pruned", its statistics zero.  Only the root's code
    // is written back: nothing reads the codes below a pruned node for anything but their (equal) scalars.
    const bool plain = tol >= 1 && cpk == 0u && tv.x == rv.x && tv.y == rv.y && tv.z == rv.z && tv.w == rv.w;
    // (RANGE: the first launch has already turned such a block's root into a 3)
    const uint32_t upC = (upB >> ((int)(niU & 3) * 2)) & 3u;
    const uint32_t myCodes = ((c4B >> ((int)(n4 & 3) * 2)) & 3u) | ((c3B >> ((int)(n3 & 3) * 2)) & 15u) | c2B | c1H |
                             ((RANGE && hU == 1 && upC == 3u) ? 0u : upC);
    if (__syncthreads_and(plain && myCodes == 0u)) {
        if (RANGE) {        // the range stream's copy of that one token
            if (t == 0) {
                cset3(CbR, ((int64_t)1 << (D - 12)) + blk);
                *((uint32_t *)(a.gapR + (int64_t)brick * a.treeCap) + (size_t)blk * PE_WORDS) = 3u;
            }
            return;
        }
        if (t == 0) {
            cset3(Cb, ((int64_t)1 << (D - 12)) + blk);
            a.subTok[(int64_t)brick * a.nEmitBlk + blk] = 1;
            *((uint32_t *)(a.gap + (int64_t)brick * a.treeCap) + (size_t)blk * PE_WORDS) = 3u;
        }
        if (t < 4) a.blockL1[(int64_t)brick * a.nEmitBlk + (size_t)blk * 4 + t] = stat_pack(0, 0, 0);
        if (t < 64) a.idxOff[(int64_t)brick * a.nIdx + (base >> 6) + t] = VR_IDX_DEAD;
        return;
    }
    // (the string buffer and the upper codes: only blocks that get here need them.  In a build without
    // k_prune_emit12_const the exact all-"keep" boxes leave above, two thirds of the bench volume's; in the default
    // build the constant ones among them have returned before the loads, so a box that loads usually gets here.
    // Barriers lie between these stores and their first readers)
    { const uint8_t cu = (uint8_t)((upB >> ((int)(niU & 3) * 2)) & 3u); codeH[t] = cu; codeOldH[t] = cu; }
#if !VR_PRUNE_CHAIN      // (otherwise waves 1 .. 3 clear it while wave 0 prunes the upper levels)
    for (int i = t; i < PE_WORDS; i += 256) W[i] = 0;
#endif
    // ---- leaves: prune (R.cpp:618-626), grown branches (R.cpp:655-704); sibling leaves share packed 16-bit lanes
    const uint32_t tw[4] = {tv.x, tv.y, tv.z, tv.w}, rw[4] = {rv.x, rv.y, rv.z, rv.w}, pwL[2] = {pv.x, pv.y};
    const uint32_t dR2 = (uint32_t)cDistR * 0x10001u, dC2 = (uint32_t)cDistC * 0x10001u;
    const uint32_t tol2 = (uint32_t)tol * 0x10001u;
    uint32_t nt[8], Lb[8];      // per lane: tokens the leaf emits when live; its code + grown branch << 2
    uint32_t bothMask = 0;
    vr_s16x2 mxB = (vr_s16x2)(0), mxA = (vr_s16x2)(0), l1p = (vr_s16x2)(0);
    const int nsteps = a.maxDepth - D;    // distanceMap[D+1..] = 64, 32, .., 1 (R.cpp:23,94-97)
    // a wave whose 1024 leaves all carry code 0 and are reproduced exactly (constant regions) prunes them all:
    // one '3' per leaf, no branches, no statistics to add
    const bool busy = __ballot(!plain) != 0ull;
    if (!busy) {
        bothMask = 0x5555u;
#pragma unroll
        for (int j = 0; j < 8; ++j) { nt[j] = 0x00010001u; Lb[j] = 0x00030003u; }
    }
    if (busy)
#pragma unroll
    for (int half = 0; half < 2; ++half) {          // two halves of four sibling pairs: halves the transient registers
        uint32_t T2[4], m[4], sg[4], act[4];
        uint32_t anyAct = 0, keepEnd = 0;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = half * 4 + jj;
            const uint32_t sel = (j & 1) ? 0x0c030c02u : 0x0c010c00u;
            T2[jj] = __builtin_amdgcn_perm(0, tw[j >> 1], sel);
            vr_s16x2 dl;
            uint32_t cl2;                                                                           // the pair's codes
            if (LEAFLESS) leaf_pair_encode(tw[j >> 1], j & 1, pwL[j >> 2], j & 3, dR2, dC2, dl, cl2);
            else {
                dl = pk_s(T2[jj]) - pk_s(__builtin_amdgcn_perm(0, rw[j >> 1], sel));
                cl2 = ((cpk >> (4 * j)) & 3u) | (((cpk >> (4 * j + 2)) & 3u) << 16);
            }
            pe_leaf_table(T2[jj], dl, cl2, tol2, [&](uint32_t k) { return lutS[k]; }, mxB, m[jj], sg[jj], act[jj], Lb[j], nt[j], bothMask, j);
            anyAct |= act[jj];
        }
        for (int i = 0; i < nsteps; ++i) {    // exact stepping for the leaves the table does not cover
            if (__ballot(anyAct != 0) == 0ull) break;
            const uint32_t d2 = (uint32_t)(64 >> i) * 0x10001u;
            anyAct = 0;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = half * 4 + jj;
                if (__ballot(act[jj] != 0u) == 0ull) continue;     // such leaves are rare: usually one pair slot of the wave at most
                pe_leaf_step(i, nsteps, d2, tol2, T2[jj], m[jj], sg[jj], act[jj], Lb[j], nt[j], keepEnd, anyAct);
            }
        }
        if (!RANGE && keepEnd) atomicAdd(&c.zeroRun, (int)((keepEnd & 1u) + ((keepEnd >> 16) & 1u)));
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) { mxA = __builtin_elementwise_max(mxA, pk_s(m[jj])); l1p += pk_s(m[jj]); }
    }
    if (!RANGE) {   // statistics (R.cpp:71-76, 115-129): one record per wave = 1024 leaves
        const int maxErr = wave_max_i32_dpp(max((int)mxB.x, (int)mxB.y)), maxAfter = wave_max_i32_dpp(max((int)mxA.x, (int)mxA.y));
        const unsigned long long l1w = (uint32_t)__builtin_amdgcn_readlane(
            (int)wave_incl_scan_add_dpp((uint32_t)((int)l1p.x + (int)l1p.y)), 63);       // < 2^18 per wave
        if ((t & 63) == 0)
            a.blockL1[(int64_t)brick * a.nEmitBlk + (size_t)blk * 4 + (t >> 6)] = stat_pack(l1w, maxErr, maxAfter);
    }
    // ---- RANGE: the leaves' tokens in the range stream.  A pruned leaf is a 3 there too (M.cpp:864-865); a live one
    // carries its own level-loop code, then as many branch nodes as the mid stream's branch has, each encodeNode
    // against the range stream's own reconstruction with the same distances (M.cpp:930-933), then the mid stream's
    // terminator if it has one
    uint32_t LbR[8];
    if (RANGE) {
        // sibling leaves in packed 16-bit lanes, like the mid stream's: per branch level one reduced encodeNode
        // (kd_common.h) for both, applied where the mid stream's branch still has an evaluated node at that level;
        // a wave leaves the level loop as soon as none of its branches is that long
        const uint32_t twR[4] = {tvR.x, tvR.y, tvR.z, tvR.w}, rwR[4] = {rvR.x, rvR.y, rvR.z, rvR.w}, pwR[2] = {pvR.x, pvR.y};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (!busy) { LbR[j] = 0x00030003u; continue; }
            const uint32_t sel = (j & 1) ? 0x0c030c02u : 0x0c010c00u;
            const vr_s16x2 T2 = pk_s(__builtin_amdgcn_perm(0, twR[j >> 1], sel));
            vr_s16x2 rec = pk_s(__builtin_amdgcn_perm(0, rwR[j >> 1], sel));
            uint32_t cR = ((cpkR >> (4 * j)) & 3u) | (((cpkR >> (4 * j + 2)) & 3u) << 16);
            if (LEAFLESS) {       // the range stream's own leaf level, recomputed like the mid stream's
                vr_s16x2 dlR;
                leaf_pair_encode(twR[j >> 1], j & 1, pwR[j >> 2], j & 3, (uint32_t)cDistRR * 0x10001u, (uint32_t)cDistCR * 0x10001u, dlR, cR);
                rec = T2 - dlR;
            }
            const uint32_t mid = Lb[j];
            const vr_s16x2 n2 = pk_s(nt[j]) - pk_s(0x00010001u);                        // branch tokens of the mid stream
            const uint32_t prunedM = ((mid & (mid >> 1)) & 0x00010001u) * 0xFFFFu;          // the leaf's own token is a 3
            vr_u16x2 lastTok = __builtin_bit_cast(vr_u16x2, mid) >> __builtin_bit_cast(vr_u16x2, n2 + n2);   // token n of each string
            const uint32_t lt = __builtin_bit_cast(uint32_t, lastTok);
            const uint32_t hasN = pk_u((vr_s16x2)(0) - n2) >> 15 & 0x00010001u;            // n > 0
            const uint32_t termB = (lt & (lt >> 1)) & hasN;                                 // bit 0 of each lane: has a terminator
            const vr_s16x2 k2 = n2 - pk_s(termB);                                           // evaluated branch nodes
            uint32_t bits = (prunedM & 0x00030003u) | (~prunedM & cR);
            for (int i = 0; i < VR_CHAIN_LEVELS; ++i) {
                const uint32_t am = pk_u((pk_s((uint32_t)i * 0x10001u) - k2) >> 15);       // 0xFFFF where k > i
                if (__ballot(am != 0u) == 0ull) break;
                const uint32_t d2 = (uint32_t)(64 >> i) * 0x10001u;
                const vr_s16x2 diff = T2 - rec, nd = (vr_s16x2)(0) - diff;
                const vr_s16x2 pd = __builtin_elementwise_max(diff, nd);
                const uint32_t up = pk_u(nd >> 15);
                const vr_s16x2 h = pk_s(pk_u(T2) ^ (up & 0x00FF00FFu));
                const vr_s16x2 x = __builtin_elementwise_min(pk_s(d2) - pd, h), ax = pk_abs(x);
                const uint32_t take = pk_u((ax - pd) >> 15) & am;
                const uint32_t code2 = take & pk_u(pk_s(up) + pk_s(0x00020002u)) & 0x00030003u;    // up ? 1 : 2
                const vr_s16x2 r = pk_mad(x, pk_mad(pk_s(up), pk_s(0xFFFEFFFEu), pk_s(0xFFFFFFFFu)), T2);   // up ? t + x : t - x
                rec = pk_s((take & pk_u(r)) | (~take & pk_u(rec)));
                bits |= code2 << (2 * i + 2);
            }
            const vr_u16x2 term = __builtin_bit_cast(vr_u16x2, termB * 3u) << __builtin_bit_cast(vr_u16x2, k2 + k2 + pk_s(0x00020002u));
            LbR[j] = bits | __builtin_bit_cast(uint32_t, term);
        }
    }
    // ---- depths D-1 .. D-4 of my 16 leaves, in registers (R.cpp:596-629: a node only depends on its children), all
    // nodes of a level at once: the eight depth-(D-1) codes sit at bits 2k, the four depth-(D-2) codes at bits 4q, the
    // two depth-(D-3) codes at bits 8r, the depth-(D-4) code at bit 0 -- a node's children are the codes at its own bit
    // position and at the next position of the finer level, so "both children are pruned tokens" is one AND of shifts
    uint32_t a1 = c1H;
    uint32_t a2 = c2B; a2 = (a2 | (a2 << 4)) & 0x0F0Fu; a2 = (a2 | (a2 << 2)) & 0x3333u;
    uint32_t a3 = (c3B >> ((int)(n3 & 3) * 2)) & 15u; a3 = (a3 | (a3 << 6)) & 0x0303u;
    uint32_t a4 = (c4B >> ((int)(n4 & 3) * 2)) & 3u;
    const auto prune_level = [](uint32_t &codes, uint32_t bothChildren, uint32_t at) -> uint32_t {
        const uint32_t keep = ~(codes | (codes >> 1)) & at;          // code == 0
        const uint32_t p = keep & bothChildren;                       // ... and both children pruned: becomes a 3
        codes |= p | (p << 1);
        return codes & (codes >> 1) & at;                             // the level's pruned tokens
    };
    const uint32_t F1 = prune_level(a1, bothMask, 0x5555u);
    const uint32_t F2 = prune_level(a2, F1 & (F1 >> 2), 0x1111u);
    const uint32_t F3 = prune_level(a3, F2 & (F2 >> 4), 0x0101u);
    const uint32_t F4 = prune_level(a4, F3 & (F3 >> 8), 0x0001u);
    // tokens a subtree emits: 1 if its root is a pruned token, else 1 + its children's
    int cnt1[8], cnt2[4], cnt3[2];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        cnt1[k] = 1 + (((int)(nt[k] & 0xFFFFu) + (int)(nt[k] >> 16)) & ~__builtin_amdgcn_sbfe((int)F1, 2 * k, 1));
#pragma unroll
    for (int q = 0; q < 4; ++q) cnt2[q] = 1 + ((cnt1[2 * q] + cnt1[2 * q + 1]) & ~__builtin_amdgcn_sbfe((int)F2, 4 * q, 1));
#pragma unroll
    for (int r = 0; r < 2; ++r) cnt3[r] = 1 + ((cnt2[2 * r] + cnt2[2 * r + 1]) & ~__builtin_amdgcn_sbfe((int)F3, 8 * r, 1));
    const int cnt4 = 1 + ((cnt3[0] + cnt3[1]) & ~__builtin_amdgcn_sbfe((int)F4, 0, 1));
#if VR_PRUNE_CHAIN
    fl4H[t] = (uint8_t)F4;
    cnt4H[t] = (uint16_t)cnt4;
    __syncthreads();
    // ---- depths D-5 .. D-12 by wave 0 in registers: 255 nodes need no workgroup barrier between their levels.  Lane l
    // reads everything it will look at in one batch -- flags and counts of the four depth-(D-4) nodes below its two
    // level-7 nodes, those two codes, and the code of its ancestor at every level above -- computes levels 7 and 6 from
    // its own registers, and from level 5 up meets its sibling subtree's (flag, count) in the lane at distance 1, 2,
    // 4, 8 (DPP; all lanes below a node hold the node's result, so any lane of the sibling's group is a partner), the
    // last two levels from the four rows' values as scalars.  Waves 1 .. 3 clear the string buffer meanwhile; the
    // barrier behind publishes both.
    if (t < 64) {
        const uint32_t fl = *(const uint32_t *)&fl4H[4 * t];
        const uint2 cn = *(const uint2 *)&cnt4H[4 * t];
        const uint32_t c7 = *(const uint16_t *)&codeH[128 + 2 * t];
        uint32_t cA[7];
#pragma unroll
        for (int lq = 0; lq < 7; ++lq) cA[lq] = codeH[(1 << lq) + (t >> (6 - lq))];
        // a node from its code and its children's (pruned flag, count): R.cpp:596-629
        const auto node = [](uint32_t code, uint32_t fL, uint32_t fR, uint32_t cL, uint32_t cR, uint32_t &f, uint32_t &cnt) -> uint32_t {
            const uint32_t nc = (fL & fR & (code == 0u ? 1u : 0u)) ? 3u : code;
            f = nc == 3u ? 1u : 0u;
            cnt = f ? 1u : 1u + cL + cR;
            return nc;
        };
        uint32_t fA, nA, fB, nB, f, n;
        const uint32_t cdA = node(c7 & 0xFFu, fl & 1u, (fl >> 8) & 1u, cn.x & 0xFFFFu, cn.x >> 16, fA, nA);
        const uint32_t cdB = node(c7 >> 8, (fl >> 16) & 1u, fl >> 24, cn.y & 0xFFFFu, cn.y >> 16, fB, nB);
        *(uint16_t *)&codeH[128 + 2 * t] = (uint16_t)(cdA | (cdB << 8));
        codeH[64 + t] = (uint8_t)node(cA[6], fA, fB, nA, nB, f, n);
        uint32_t v = n | (f << 16);              // a count is at most 36863
#pragma unroll
        for (int lq = 5; lq >= 2; --lq) {
            const uint32_t pv = lq == 5 ? dpp_u32<0xB1, 0xf>(v, v)        // quad_perm [1,0,3,2]
                              : lq == 4 ? dpp_u32<0x4E, 0xf>(v, v)        // quad_perm [2,3,0,1]
                              : lq == 3 ? dpp_u32<0x141, 0xf>(v, v)       // row_half_mirror: the other quad of my eight
                                        : dpp_u32<0x140, 0xf>(v, v);      // row_mirror: the other eight of my row
            const uint32_t nc = node(cA[lq], v >> 16, pv >> 16, v & 0xFFFFu, pv & 0xFFFFu, f, n);
            v = n | (f << 16);
            if (nc != cA[lq] && (t & ((2 << (5 - lq)) - 1)) == 0) codeH[(1 << lq) + (t >> (6 - lq))] = 3;
        }
        // levels 1 and 0: the four rows' results and the three codes are wave-uniform
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
        const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
        const uint32_t k2 = (uint32_t)__builtin_amdgcn_readlane((int)cA[1], 0), k3 = (uint32_t)__builtin_amdgcn_readlane((int)cA[1], 32);
        const uint32_t k1 = (uint32_t)__builtin_amdgcn_readlane((int)cA[0], 0);
        uint32_t f2, n2h, f3, n3h, f1, n1h;
        const uint32_t cd2 = node(k2, r0 >> 16, r1 >> 16, r0 & 0xFFFFu, r1 & 0xFFFFu, f2, n2h);
        const uint32_t cd3 = node(k3, r2 >> 16, r3 >> 16, r2 & 0xFFFFu, r3 & 0xFFFFu, f3, n3h);
        const uint32_t cd1 = node(k1, f2, f3, n2h, n3h, f1, n1h);
        if (t == 0) {
            codeH[1] = (uint8_t)cd1; codeH[2] = (uint8_t)cd2; codeH[3] = (uint8_t)cd3;
            if (!RANGE) a.subTok[(int64_t)brick * a.nEmitBlk + blk] = n1h;
        }
    } else {
        for (int i = t - 64; i < PE_WORDS / 4; i += 192) ((uint4 *)W)[i] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
#else
    flH[256 + t] = (uint8_t)F4;
    cntH[256 + t] = (uint16_t)cnt4;
    __syncthreads();
    // ---- depths D-5 .. D-12 in LDS
    for (int lq = 7; lq >= 0; --lq) {
        if (t < (1 << lq)) {
            const int h = (1 << lq) + t;
            const uint32_t code = codeH[h];
            const bool p = flH[2 * h] && flH[2 * h + 1] && code == 0;
            if (p) codeH[h] = 3;
            const bool f = p || code == 3;
            flH[h] = (uint8_t)(f ? 1 : 0);
            cntH[h] = (uint16_t)(f ? 1u : 1u + cntH[2 * h] + cntH[2 * h + 1]);
        }
        __syncthreads();
    }
#endif
    // RANGE: from here on the token VALUES are the range stream's: its own codes, 3 wherever the mid stream pruned
    // (M.cpp:864-865); the shape (which tokens exist) is unchanged because a token is 3 in both streams or in neither
    if (RANGE) {
        const auto merge = [](uint32_t mid, uint32_t rng) { const uint32_t m3 = (mid & (mid >> 1) & 0x55555555u) * 3u; return (rng & ~m3) | m3; };
        uint32_t r2 = c2BR; r2 = (r2 | (r2 << 4)) & 0x0F0Fu; r2 = (r2 | (r2 << 2)) & 0x3333u;      // spread like a2, a3
        uint32_t r3 = (c3BR >> ((int)(n3 & 3) * 2)) & 15u; r3 = (r3 | (r3 << 6)) & 0x0303u;
        a1 = merge(a1, c1HR) & 0xFFFFu;
        a2 = merge(a2, r2) & 0x3333u;
        a3 = merge(a3, r3) & 0x0303u;
        a4 = merge(a4, (c4BR >> ((int)(n4 & 3) * 2)) & 3u) & 3u;
        const uint8_t ro = (uint8_t)((upBR >> ((int)(niU & 3) * 2)) & 3u);
        const uint8_t mc = codeH[t];
        __syncthreads();
        codeOldH[t] = ro;
        codeH[t] = mc == 3 ? (uint8_t)3 : ro;
#pragma unroll
        for (int j = 0; j < 8; ++j) Lb[j] = LbR[j];
        __syncthreads();
    }
    uint8_t *Cw = RANGE ? CbR : Cb;
    // the BFS codes are read again only down to depth Ds = D-6 (upper prune levels, k_block_alive, k_concat12's
    // index values, progressive cuts): write back depths D-12 .. D-5; below that they are dead from here on
    if (t >= 1 && t < 64) {                               // heap bytes 1..63 <-> heap nodes 4..255 (whole bytes are mine)
        const int h = t * 4, lq = 31 - __clz(h);
        const uint8_t pk = (uint8_t)(codeH[h] | (codeH[h + 1] << 2) | (codeH[h + 2] << 4) | (codeH[h + 3] << 6));
        const uint8_t po = (uint8_t)(codeOldH[h] | (codeOldH[h + 1] << 2) | (codeOldH[h + 2] << 4) | (codeOldH[h + 3] << 6));
        if (pk != po) Cw[(((int64_t)1 << (D - 12 + lq)) + ((int64_t)blk << lq) + (h - (1 << lq))) >> 2] = pk;
    }
    if (t >= 1 && t < 4 && codeH[t] != codeOldH[t]) {     // heap nodes 1..3 share bytes with neighbouring blocks
        const int lq = 31 - __clz(t);
        cset3(Cw, ((int64_t)1 << (D - 12 + lq)) + ((int64_t)blk << lq) + (t - (1 << lq)));
    }
#if !VR_PRUNE_CHAIN      // (otherwise wave 0 wrote it from its register)
    if (!RANGE && t == 0) a.subTok[(int64_t)brick * a.nEmitBlk + blk] = cntH[1];
#endif
    // ---- top-down: the block's own token string, root assumed live.  Thread t owns the live nodes whose
    // first leaf is its first leaf: ancestors at in-block level lq (depth D-12+lq) when t % 2^(8-lq) == 0
    const int jmin = t ? 8 - (__ffs(t) - 1) : 0;
    bool alive = true;
    if (jmin > 0) alive = codeH[(1 << (jmin - 1)) + (t >> (9 - jmin))] != 3;       // parent not pruned
    uint32_t S = 0;
    int ns = 0, preDs = 0, aliveAtDs = 0;
    for (int lq = jmin; lq <= 7 && alive; ++lq) {
        if (lq == 6) { preDs = ns; aliveAtDs = 1; }
        const uint32_t code = codeH[(1 << lq) + (t >> (8 - lq))];
        S |= code << (2 * ns);
        ++ns;
        if (code == 3) alive = false;
    }
    uint32_t tot;
    const uint32_t pos = block4_excl_scan_u32((uint32_t)(ns + (alive ? cnt4 : 0)), shw, tot);
    uint32_t bitpos = 2u * pos;
    pe_put(W, bitpos, (unsigned long long)S, ns);
    bitpos += 2u * (uint32_t)ns;
    if (alive) {
        // preorder of my 31-node subtree; internal tokens wait in (pb, pn) and leave with the next leaf-pair piece
        unsigned long long pb = a4;
        int pn = 1;
        if (a4 != 3u) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint32_t c3 = (a3 >> (8 * r)) & 3u;
                pb |= (unsigned long long)c3 << (2 * pn); ++pn;
                if (c3 == 3u) continue;
#pragma unroll
                for (int qq = 0; qq < 2; ++qq) {
                    const int q = 2 * r + qq;
                    const uint32_t c2 = (a2 >> (4 * q)) & 3u;
                    pb |= (unsigned long long)c2 << (2 * pn); ++pn;
                    if (c2 == 3u) continue;
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        const int k = 2 * q + kk;
                        const uint32_t c1 = (a1 >> (2 * k)) & 3u;
                        unsigned long long H = c1;
                        int Hn = 1;
                        if (c1 != 3u) {
                            const int n0 = (int)(nt[k] & 0xFFFFu), n1t = (int)(nt[k] >> 16);
                            H |= ((unsigned long long)(Lb[k] & 0xFFFFu) << 2) | ((unsigned long long)(Lb[k] >> 16) << (2 + 2 * n0));
                            Hn = 1 + n0 + n1t;
                        }
                        pe_put(W, bitpos, pb | (H << (2 * pn)), pn + Hn);
                        bitpos += 2u * (uint32_t)(pn + Hn);
                        pb = 0; pn = 0;
                    }
                }
            }
        }
        pe_put(W, bitpos, pb, pn);
    }
    if (!RANGE && (t & 3) == 0)       // decode side-car index: the depth-Ds node of every 64 leaves, block-local for now
        a.idxOff[(int64_t)brick * a.nIdx + (base >> 6) + (t >> 2)] = aliveAtDs ? pos + (uint32_t)preDs : VR_IDX_DEAD;
    if (!RANGE) {
        // ... and, below it, how many tokens each 4-leaf subtree owns in preorder: its own nodes plus the
        // ancestors (depth >= Ds) whose first leaf is its first leaf.  One byte each (at most 4 + 39 tokens); the
        // decoder turns them into token offsets with a 16-lane prefix sum, so one lane decodes four voxels.
        const int nsIn = jmin <= 6 ? (aliveAtDs ? ns - preDs : 0) : ns;
        const bool l4 = alive && a4 != 3u;
        const bool l30 = l4 && (a3 & 3u) != 3u, l31 = l4 && ((a3 >> 8) & 3u) != 3u;
        const uint32_t f0 = (uint32_t)(nsIn + (alive ? 1 + (l4 ? 1 + (l30 ? cnt2[0] : 0) : 0) : 0));
        const uint32_t f1 = (uint32_t)(l30 ? cnt2[1] : 0);
        const uint32_t f2 = (uint32_t)(l4 ? 1 + (l31 ? cnt2[2] : 0) : 0);
        const uint32_t f3 = (uint32_t)(l31 ? cnt2[3] : 0);
        a.fineIdx[((int64_t)brick * a.nIdx + (base >> 6)) * 4 + t] = f0 | (f1 << 8) | (f2 << 16) | (f3 << 24);
    }
    __syncthreads();
    // the block's slot of the gapped stream buffer; one word past the string too, so that no stale token of an earlier
    // build sits right behind it (the decoders fetch whole words past a run's end; what they fetch there is never used)
    const uint32_t nw = min((tot + 15u) / 16u + 1u, (uint32_t)PE_WORDS);
    uint32_t *slot = (uint32_t *)((RANGE ? a.gapR : a.gap) + (int64_t)brick * a.treeCap) + (size_t)blk * PE_WORDS;
    for (uint32_t i = t; i < nw; i += 256u) slot[i] = W[i];
}


// ---- constant 4096-leaf blocks (flag bit 0 of k_pyramid12) of a leafless SkipBlocks build: closed form ----------
// By induction from its root such a block is uniform: every node of a level has the same truth, the same parent
// reconstruction, hence the same code and error, and every leaf grows the same branch.  What k_prune_emit12 computes
// for it is a function of a few scalars -- the value, one code per level, the leaf's parent reconstruction, the two
// final distances -- and this kernel writes the same bytes from them: one leaf pair through the leaf stage's own code
// (leaf_pair_encode, pe_leaf_table, pe_leaf_step), the bottom-up prune (R.cpp:596-629) on twelve scalars, and the
// string, the preorder of a perfect tree with one token per level, at closed-form positions: thread t's tokens start
// at t * len[8] + sum over the live in-block levels lq <= 7 of ceil(t / 2^(8-lq)) -- no scan, no prune levels in LDS.
// A workgroup takes PEC_BOXES consecutive blocks: one batch of scalar loads, one lane per block for the chain, the
// one-token blocks (two thirds of all constant ones) written by a few lanes each, the others composed one after the other:
// the 16-leaf subtree, one string for all 256 threads, is made once and shifted to each thread's position.
// k_prune_emit12<false, true> returns on the blocks this kernel owns (PruneEmitArgs::uniformBlocks).
#ifndef PEC_BOXES
#define PEC_BOXES 16
#endif
__global__ void __launch_bounds__(256)
k_prune_emit12_const(PruneEmitArgs a)
{
    __shared__ uint32_t lutS[512];
    __shared__ uint32_t W[PE_WORDS];
    // per block: the codes of in-block levels 0 .. 11, [12] the value, [13] the leaves' parent reconstruction, [14] the flags
    __shared__ __attribute__((aligned(16))) uint8_t sc[PEC_BOXES][16];
    __shared__ uint32_t res[PEC_BOXES][6];
    __shared__ uint32_t Pc[12];                       // the 16-leaf subtree's string (at most 159 tokens), zero behind it
    const int brick = blockIdx.y, t = threadIdx.x, D = a.D, tol = a.tol;
    Ctrl &c = a.ctrls[brick];
    const int cConst = c.constBrick, cRa = c.ra, cDistR = c.finalReconDist, cDistC = c.finalCodesDist;     // one scalar round trip
    if (cConst) return;
    const uint32_t nBlk = (uint32_t)a.sk.nBlk, blk0 = blockIdx.x * (uint32_t)PEC_BOXES;
    uint8_t *Cb = a.codes + (int64_t)brick * a.codeStride;
    const uint8_t *Tb = a.temp + (int64_t)brick * a.heapStride;
    const uint8_t *Pb = (cRa == 0 ? a.rb.b[0] : (cRa == 1 ? a.rb.b[1] : a.rb.b[2])) + (int64_t)brick * a.leafStride;
    lutS[t] = a.chainLut[VR_CHAIN_LUT_SIGNED + t]; lutS[256 + t] = a.chainLut[VR_CHAIN_LUT_SIGNED + 256 + t];
    // ---- the blocks' scalars.  A skipped block (bit 1) has nothing in memory at depths D-1 and D: "keep" and exact
    for (int i = t; i < PEC_BOXES * 16; i += 256) {
        const int b = i >> 4, l = i & 15;
        const uint32_t blk = blk0 + (uint32_t)b;
        uint32_t val = 0;
        if (blk < nBlk) {
            const uint32_t f = a.sk.flag[(int64_t)brick * a.sk.nBlk + blk];
            const bool filled = (f & 3u) == 1u;
            if (l == 14) val = f;
            else if (f & 1u) {
                if (l < 11 || (l == 11 && filled)) val = (uint32_t)cget(Cb, ((int64_t)1 << (D - 12 + l)) + ((int64_t)blk << l));
                else if (l == 12) val = Tb[((int64_t)1 << (D - 12)) + blk];
                else if (l == 13 && filled) val = Pb[(int64_t)blk << 11];
            }
        }
        sc[b][l] = (uint8_t)val;
    }
    __syncthreads();
    // ---- one lane per block: leaf, prune, subtree lengths
    if (t < PEC_BOXES) {
        const uint4 q = *(const uint4 *)sc[t];
        const uint32_t f = (q.w >> 16) & 255u;
        uint32_t kind = 0;                                  // 0: not mine, 1: the one-token early exit, 2: a string
        if (f & 1u) {
            const bool filled = (f & 3u) == 1u;
            const uint32_t v = q.w & 255u, p = filled ? (q.w >> 8) & 255u : v;
            uint32_t uc = 0;                                // the twelve codes, level l at bits 2l
#pragma unroll
            for (int l = 0; l < 12; ++l) uc |= (((l < 4 ? q.x : (l < 8 ? q.y : q.z)) >> (8 * (l & 3))) & 3u) << (2 * l);
            const uint32_t tword = v * 0x01010101u, pword = p * 0x01010101u, tol2 = (uint32_t)tol * 0x10001u;
            vr_s16x2 dl, mxB = (vr_s16x2)(0);
            uint32_t cl2, m, sg, act, Lb, nt, keepEnd = 0;
            leaf_pair_encode(tword, 0, pword, 0, (uint32_t)cDistR * 0x10001u, (uint32_t)cDistC * 0x10001u, dl, cl2);
            const uint32_t T2 = __builtin_amdgcn_perm(0, tword, 0x0c010c00u);
            uint32_t both = 0;                              // bit 0: the leaf is a pruned token
            pe_leaf_table(T2, dl, cl2, tol2, [&](uint32_t k) { return lutS[k]; }, mxB, m, sg, act, Lb, nt, both, 0);
            const int nsteps = a.maxDepth - D;
            uint32_t anyAct = act;
            for (int i = 0; i < nsteps && anyAct; ++i) {
                anyAct = 0;
                pe_leaf_step(i, nsteps, (uint32_t)(64 >> i) * 0x10001u, tol2, T2, m, sg, act, Lb, nt, keepEnd, anyAct);
            }
            const bool early = v == p && uc == 0u;          // what k_prune_emit12 leaves on before its string buffer
            bool F = both != 0u;
            uint32_t len = nt & 0xFFFFu, len8 = 0, len10 = 0, changed = 0, P = 12;
#pragma unroll
            for (int l = 11; l >= 0; --l) {
                if (F && ((uc >> (2 * l)) & 3u) == 0u) { uc |= 3u << (2 * l); changed |= 1u << l; }
                F = ((uc >> (2 * l)) & 3u) == 3u;
                len = F ? 1u : 1u + 2u * len;
                if (F) P = (uint32_t)l;
                if (l == 10) len10 = len;
                if (l == 8) len8 = len;
            }
            kind = early ? 1u : 2u;
            res[t][1] = uc;
            res[t][2] = (Lb & 0xFFFFu) | ((nt & 0xFFFFu) << 16);
            res[t][3] = len8 | (len10 << 16);
            res[t][4] = len;
            res[t][5] = (m & 0xFFFFu) | ((uint32_t)(int)mxB.x << 16);
            res[t][0] = kind | (P << 4) | (changed << 8) | ((keepEnd & 1u) << 20);
        } else
            res[t][0] = 0;
    }
    __syncthreads();
    // ---- the one-token blocks: root code 3, one token, zero statistics, 64 dead index entries
    for (int i = t; i < PEC_BOXES * 16; i += 256) {
        const int b = i >> 4, l = i & 15;
        if ((res[b][0] & 15u) != 1u) continue;
        const uint32_t blk = blk0 + (uint32_t)b;
        *(uint4 *)(a.idxOff + (int64_t)brick * a.nIdx + ((int64_t)blk << 6) + l * 4) = make_uint4(VR_IDX_DEAD, VR_IDX_DEAD, VR_IDX_DEAD, VR_IDX_DEAD);
        if (l < 4) a.blockL1[(int64_t)brick * a.nEmitBlk + (size_t)blk * 4 + l] = stat_pack(0, 0, 0);
        if (l == 0) {
            cset3(Cb, ((int64_t)1 << (D - 12)) + blk);
            a.subTok[(int64_t)brick * a.nEmitBlk + blk] = 1;
            *((uint32_t *)(a.gap + (int64_t)brick * a.treeCap) + (size_t)blk * PE_WORDS) = 3u;
        }
    }
    // ---- the others, one after the other
    const int jmin = t ? 8 - (__ffs(t) - 1) : 0;
    for (int b = 0; b < PEC_BOXES; ++b) {
        const uint32_t r0 = res[b][0];
        if ((r0 & 15u) != 2u) continue;                     // (the same answer in every thread)
        const uint32_t blk = blk0 + (uint32_t)b, base = blk << 12;
        const int P = (int)((r0 >> 4) & 15u);
        const uint32_t changed = (r0 >> 8) & 0xFFFu, uc = res[b][1], LbL = res[b][2] & 0xFFFFu, ntL = res[b][2] >> 16;
        const uint32_t len8 = res[b][3] & 0xFFFFu, len10 = res[b][3] >> 16, tot = res[b][4];
        const uint32_t nw = min((tot + 15u) / 16u + 1u, (uint32_t)PE_WORDS);
        for (uint32_t i = t; i < nw; i += 256u) W[i] = 0;
        if (t < 12) Pc[t] = 0;
        // code write-back, depths D-12 .. D-5, by k_prune_emit12's rule: whole bytes below heap node 3, bits above
        if (t >= 1 && t < 64) {
            const int h = t * 4, lq = 31 - __clz(h);
            if ((changed >> lq) & 1u) Cb[(((int64_t)1 << (D - 12 + lq)) + ((int64_t)blk << lq) + (h - (1 << lq))) >> 2] = 0xFFu;
        }
        if (t >= 1 && t < 4) {
            const int lq = 31 - __clz(t);
            if ((changed >> lq) & 1u) cset3(Cb, ((int64_t)1 << (D - 12 + lq)) + ((int64_t)blk << lq) + (t - (1 << lq)));
        }
        if (t == 0) {
            a.subTok[(int64_t)brick * a.nEmitBlk + blk] = tot;
            a.boxUniform[(int64_t)brick * a.sk.nBlk + blk] = 1u;     // uniform by induction: one byte per cut (k_decode_region)
        }
        if (t < 4) {
            const uint32_t fe = res[b][5] & 0xFFFFu, eB = res[b][5] >> 16;
            a.blockL1[(int64_t)brick * a.nEmitBlk + (size_t)blk * 4 + t] = stat_pack((unsigned long long)fe * 1024ull, (int)eB, (int)fe);
        }
        if ((r0 >> 20) & 1u) atomicAdd(&c.zeroRun, 4);     // (k_prune_emit12: two per thread and half of its leaves)
        __syncthreads();
        // thread t: the live ancestors whose first leaf is its first leaf, then its 16-leaf subtree
        const int top = P < 7 ? P : 7;
        const int ns = jmin <= top ? top - jmin + 1 : 0;
        uint32_t pos = P >= 8 ? (uint32_t)t * len8 : 0u;
        for (int lq = 0; lq <= top; ++lq) pos += ((uint32_t)t + (1u << (8 - lq)) - 1u) >> (8 - lq);
        uint32_t bitpos = 2u * pos;
        pe_put(W, bitpos, (unsigned long long)((uc >> (2 * jmin)) & ((1u << (2 * ns)) - 1u)), ns);
        bitpos += 2u * (uint32_t)ns;
        // a subtree that reaches its leaf pairs is the same string for every thread: eight threads write one pair's
        // piece each into Pc, and after a barrier every thread shifts the whole string to its own position
        if (P >= 11 && t < 8) {
            const uint32_t a4 = (uc >> 16) & 3u, a3 = (uc >> 18) & 3u, a2 = (uc >> 20) & 3u, a1 = (uc >> 22) & 3u;
            unsigned long long H = a1;
            int Hn = 1;
            if (a1 != 3u) { H |= ((unsigned long long)LbL << 2) | ((unsigned long long)LbL << (2 + 2 * ntL)); Hn = 1 + 2 * (int)ntL; }
            // internal tokens in front of pair t: a4 a3 a2 | - | a2 | - | a3 a2 | - | a2 | -
            const int pn = (int)((0x01020103u >> (4 * t)) & 15u);
            const int pre = (0x76644330u >> (4 * t)) & 15;                      // ... and in front of those, over pairs 0 .. t-1
            const uint32_t pb = t == 0 ? a4 | (a3 << 2) | (a2 << 4) : (t == 4 ? a3 | (a2 << 2) : a2);
            pe_put(Pc, 2u * (uint32_t)(pre + t * Hn), (unsigned long long)(pn ? pb : 0u) | (H << (2 * pn)), pn + Hn);
        }
        if (P >= 8 && P < 11) {                             // pruned above the pairs: a4 | a4 a3 a3 | a4 a3 a2 a2 a3 a2 a2
            const uint32_t a4 = (uc >> 16) & 3u, a3 = (uc >> 18) & 3u, a2 = (uc >> 20) & 3u;
            const uint32_t pc = P == 8 ? a4 : (P == 9 ? a4 | (a3 * 0x14u) : a4 | (a3 * 0x104u) | (a2 * 0x1450u));
            pe_put(W, bitpos, (unsigned long long)pc, (int)len8);
        }
        if (P >= 11) {                                      // (the same answer in every thread)
            __syncthreads();
            const uint32_t b1 = bitpos + 2u * len8 - 1u, w0 = bitpos >> 5, w1 = b1 >> 5, sh = bitpos & 31u;
            uint32_t lo = 0;
            for (uint32_t w = w0; w <= w1; ++w) {
                const uint32_t hi = Pc[w - w0];
                const uint32_t val = sh ? (hi << sh) | (lo >> (32u - sh)) : hi;
                lo = hi;
                // the words in between are this thread's alone; its first and last one it shares with its neighbours
                if (w == w0 || w == w1) atomicOr(&W[w], val); else W[w] = val;
            }
        }
        if ((t & 3) == 0)
            a.idxOff[(int64_t)brick * a.nIdx + (base >> 6) + (t >> 2)] = P >= 6 ? pos + (uint32_t)(6 - jmin) : VR_IDX_DEAD;
        {
            const uint32_t nsIn = jmin <= 6 ? (P >= 6 ? (uint32_t)(top - 5) : 0u) : (uint32_t)ns;
            const bool alive = P >= 8, l4 = P >= 9, l3 = P >= 10;
            const uint32_t f0 = nsIn + (alive ? 1u + (l4 ? 1u + (l3 ? len10 : 0u) : 0u) : 0u);
            const uint32_t f1 = l3 ? len10 : 0u;
            const uint32_t f2 = l4 ? 1u + (l3 ? len10 : 0u) : 0u;
            a.fineIdx[((int64_t)brick * a.nIdx + (base >> 6)) * 4 + t] = f0 | (f1 << 8) | (f2 << 16) | (f1 << 24);
        }
        __syncthreads();
        uint32_t *slot = (uint32_t *)(a.gap + (int64_t)brick * a.treeCap) + (size_t)blk * PE_WORDS;
        for (uint32_t i = t; i < nw; i += 256u) slot[i] = W[i];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(EMIT_RANKS_PER_BLOCK)
k_emit_count(EmitArgs a)
{
    __shared__ uint32_t shw[4];
    const int brick = blockIdx.y;
    const Ctrl &c = a.ctrls[brick];
    if (c.constBrick) return;
    const uint8_t *Cb = a.codes + (int64_t)brick * a.codeStride;
    const uint8_t *Tb = a.temp + (int64_t)brick * a.heapStride;
    const uint8_t *Rl = a.rb.b[c.par] + (int64_t)brick * a.leafStride;
    const uint32_t n = 1u << a.D;
    uint32_t r = blockIdx.x * EMIT_RANKS_PER_BLOCK + threadIdx.x;
    uint32_t w = 0;
    if (r < n) {
        Owned o = owned_tokens(Cb, nullptr, Tb, nullptr, Rl, nullptr, a.D, a.maxDepth, a.tol, c.distanceMap, nullptr,
                               a.Ds, r);
        w = o.nSpine + o.nLeaf;
    }
    uint32_t tot;
    block_excl_scan_u32(w, shw, tot);
    if (threadIdx.x == 0) a.blockTot[(int64_t)brick * a.nEmitBlk + blockIdx.x] = tot;
}

// exclusive scan of the per-block token counts of one brick (one block per brick)
__global__ void __launch_bounds__(1024)
k_emit_scan(EmitArgs a, int64_t nblk)
{
    __shared__ uint32_t shw[16];
    __shared__ unsigned long long carrySh;
    const int brick = blockIdx.x;
    if (a.ctrls[brick].constBrick) return;
    const uint32_t *in = a.blockTot + (int64_t)brick * a.nEmitBlk;
    uint32_t *out = a.blockOff + (int64_t)brick * a.nEmitBlk;
    unsigned long long *out64 = a.blockOff64 ? a.blockOff64 + (int64_t)brick * a.nEmitBlk : nullptr;
    if (threadIdx.x == 0) carrySh = 0;
    __syncthreads();
    for (int64_t base = 0; base < nblk; base += 1024) {
        int64_t i = base + threadIdx.x;
        uint32_t v = i < nblk ? in[i] : 0;
        uint32_t tot;
        uint32_t ex = block_excl_scan_u32(v, shw, tot);        // 1024 blocks of at most 9 * 4096 tokens: fits 32 bits
        unsigned long long carry = carrySh;
        if (i < nblk) { out[i] = (uint32_t)(carry + ex); if (out64) out64[i] = carry + ex; }
        __syncthreads();
        if (threadIdx.x == 0) carrySh = carry + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.ctrls[brick].numActive = carrySh;     // numActiveNodes (R.cpp:714)
        if (a.ctrlsR) a.ctrlsR[brick].numActive = carrySh;
    }
}

// Words that contain a block boundary are merged with atomicOr; they are zeroed here
// first (every shared word is the first or last word of some block's token range).
__global__ void __launch_bounds__(256)
k_emit_zero(EmitArgs a, int64_t nblk)
{
    const int brick = blockIdx.y;
    int64_t blk = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (blk >= nblk || a.ctrls[brick].constBrick) return;
    if (a.brickOff && a.brickOff[gridDim.y] > (unsigned long long)a.compactCap) return;       // (did not fit: nothing is written)
    const unsigned long long g0 = a.blockOff64 ? a.blockOff64[(int64_t)brick * a.nEmitBlk + blk] : a.blockOff[(int64_t)brick * a.nEmitBlk + blk];
    uint32_t tot = a.blockTot[(int64_t)brick * a.nEmitBlk + blk];
    const int64_t base = a.brickOff ? (int64_t)a.brickOff[brick] : (int64_t)brick * a.treeCap;
    uint32_t *W = (uint32_t *)(a.tree + base);
    uint32_t *WR = a.treeR ? (uint32_t *)(a.treeR + base) : nullptr;
    if (tot == 0) {
        if (blk == 0 && a.ctrls[brick].numActive == 0) { W[0] = 0; if (WR) WR[0] = 0; }
        return;
    }
    W[g0 >> 4] = 0;
    W[(g0 + tot - 1) >> 4] = 0;
    if (WR) { WR[g0 >> 4] = 0; WR[(g0 + tot - 1) >> 4] = 0; }
}

// byte offset of every brick's contiguous stream in the compact buffers (16-byte aligned, one spare word each) and
// their total; the streams of all bricks back to back take what they take, not B times the worst case
__global__ void __launch_bounds__(1024)
k_brick_offsets(const Ctrl *ctrls, int B, unsigned long long *brickOff, int64_t cap, int32_t *overflow)
{
    __shared__ unsigned long long part[16];
    __shared__ unsigned long long carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < B; base += 1024) {
        const int b = base + t;
        unsigned long long bytes = 0;
        if (b < B) bytes = ((((ctrls[b].numActive + 15ull) >> 4) + 1ull) * 4ull + 15ull) & ~15ull;
        unsigned long long incl = bytes;
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long n = __shfl_up(incl, o); if ((t & 63) >= o) incl += n; }
        if ((t & 63) == 63) part[t >> 6] = incl;
        __syncthreads();
        unsigned long long before = carry;
        for (int i = 0; i < (t >> 6); ++i) before += part[i];
        if (b < B) brickOff[b] = before + incl - bytes;
        __syncthreads();
        if (t == 1023) carry = before + incl;
        __syncthreads();
    }
    if (t == 0) { brickOff[B] = carry; *overflow = carry > (unsigned long long)cap ? 1 : 0; }
}

#define EMIT_LDS_WORDS 256   // 4096 tokens >= 256*9 + 511 + 32 (+15 phase)

__device__ inline void lds_put(uint32_t *W, uint32_t pos, uint32_t bits, int ntok)
{
    if (ntok <= 0) return;
    unsigned long long v = (unsigned long long)bits << ((pos & 15u) * 2u);
    uint32_t w = pos >> 4;
    atomicOr(&W[w], (uint32_t)v);
    uint32_t hi = (uint32_t)(v >> 32);
    if (hi) atomicOr(&W[w + 1], hi);
}

__global__ void __launch_bounds__(EMIT_RANKS_PER_BLOCK)
k_emit_write(EmitArgs a)
{
    __shared__ uint32_t shw[4];
    __shared__ uint32_t W[EMIT_LDS_WORDS], WR[EMIT_LDS_WORDS];
    const int brick = blockIdx.y;
    Ctrl &c = a.ctrls[brick];
    if (c.constBrick) return;
    const bool mr = a.codesR != nullptr;
    const uint8_t *Cb = a.codes + (int64_t)brick * a.codeStride;
    const uint8_t *Tb = a.temp + (int64_t)brick * a.heapStride;
    const uint8_t *Rl = a.rb.b[c.par] + (int64_t)brick * a.leafStride;
    const uint8_t *CbR = mr ? a.codesR + (int64_t)brick * a.codeStride : nullptr;
    const uint8_t *TbR = mr ? a.tempR + (int64_t)brick * a.heapStride : nullptr;
    const uint8_t *RlR = mr ? a.rbR.b[a.ctrlsR[brick].par] + (int64_t)brick * a.leafStride : nullptr;
    const uint8_t *dmapR = mr ? a.ctrlsR[brick].distanceMap : nullptr;
    const uint32_t n = 1u << a.D;
    const uint32_t r = blockIdx.x * EMIT_RANKS_PER_BLOCK + threadIdx.x;
    for (int i = threadIdx.x; i < EMIT_LDS_WORDS; i += blockDim.x) { W[i] = 0; WR[i] = 0; }
    Owned o;
    o.nSpine = o.nLeaf = 0; o.finalErr = -1; o.aliveAtDs = 0; o.preDs = 0; o.zeroRun = 0;
    if (r < n) o = owned_tokens(Cb, CbR, Tb, TbR, Rl, RlR, a.D, a.maxDepth, a.tol, c.distanceMap, dmapR, a.Ds, r);
    if (o.zeroRun) atomicAdd(&c.zeroRun, 1);
    uint32_t w = o.nSpine + o.nLeaf, tot;
    uint32_t lo = block_excl_scan_u32(w, shw, tot); // also orders the LDS clear above
    const uint32_t g0 = a.blockOff[(int64_t)brick * a.nEmitBlk + blockIdx.x];
    const uint32_t phase = g0 & 15u;
    if (w) {
        uint32_t pos = phase + lo;
        lds_put(W, pos, (uint32_t)o.spineBits, o.nSpine < 16 ? o.nSpine : 16);
        if (o.nSpine > 16) lds_put(W, pos + 16, (uint32_t)(o.spineBits >> 32), o.nSpine - 16);
        lds_put(W, pos + o.nSpine, o.leafBits, o.nLeaf);
        if (mr) {
            lds_put(WR, pos, (uint32_t)o.spineBitsR, o.nSpine < 16 ? o.nSpine : 16);
            if (o.nSpine > 16) lds_put(WR, pos + 16, (uint32_t)(o.spineBitsR >> 32), o.nSpine - 16);
            lds_put(WR, pos + o.nSpine, o.leafBitsR, o.nLeaf);
        }
    }
    // decode side-car index: one entry per depth-Ds subtree root
    if (r < n && (r & ((1u << a.K) - 1u)) == 0) {
        const uint32_t s = r >> a.K;
        int val = c.distanceMap[0];              // root scalar (R.cpp:743)
        for (int j = 1; j <= a.Ds; ++j) {
            int code = cget(Cb, ((int64_t)1 << j) + (s >> (a.Ds - j)));
            val = apply_code(val, code, c.distanceMap[j]); // pruned descendants carry code 3: unchanged
        }
        a.idxOff[(int64_t)brick * a.nIdx + s] = o.aliveAtDs ? g0 + lo + (uint32_t)o.preDs : VR_IDX_DEAD;
        a.idxVal[(int64_t)brick * a.nIdx + s] = (uint8_t)val;
    }
    __syncthreads();
    if (tot == 0) return;
    uint32_t *G = (uint32_t *)(a.tree + (int64_t)brick * a.treeCap) + (g0 >> 4);
    uint32_t *GR = mr ? (uint32_t *)(a.treeR + (int64_t)brick * a.treeCap) + (g0 >> 4) : nullptr;
    const uint32_t nw = ((phase + tot - 1) >> 4) + 1;
    for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) {
        if (i == 0 || i == nw - 1) { if (W[i]) atomicOr(&G[i], W[i]); if (mr && WR[i]) atomicOr(&GR[i], WR[i]); }
        else { G[i] = W[i]; if (mr) GR[i] = WR[i]; }
    }
}

// One flag per emit block of 2^sub leaves (a 4096-leaf block of k_prune_emit12): does its depth-(D-sub) subtree emit
// anything at all?  No iff a proper ancestor of that subtree's root was pruned and this block does not hold that
// ancestor's first leaf (the pruned ancestor's own token belongs to the block that does).  Lets k_index12 and
// k_concat12 skip the constant regions of a volume.
__global__ void __launch_bounds__(256)
k_block_alive(EmitArgs a, int64_t nblk, int sub)     // sub: log2 of the leaves per emit block (always 12)
{
    const int brick = blockIdx.y;
    const int64_t blk = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (blk >= nblk || a.ctrls[brick].constBrick) return;
    const uint8_t *Cb = a.codes + (int64_t)brick * a.codeStride;
    const uint8_t *dmap = a.ctrls[brick].distanceMap;
    const int dl = a.D - sub;
    bool alive = true;
    int val = dmap[0];                       // decoded scalar along the path (root: R.cpp:743)
    unsigned long long spine = 0, spineR = 0; // tokens above depth D-sub owned by the block's first rank (mid / range stream)
    const uint8_t *CbR = a.codesR ? a.codesR + (int64_t)brick * a.codeStride : nullptr;
    int nsp = 0;
    const uint32_t r0 = (uint32_t)blk << sub;
    const int jmin = r0 ? a.D - (__ffs((int)r0) - 1) : 0;     // first spine depth of rank r0 (<= dl)
    bool pathAlive = true;
    for (int j = 0; j < dl; ++j) {
        const int code = cget(Cb, ((int64_t)1 << j) + (blk >> (dl - j)));
        if (j > 0) val = apply_code(val, code, dmap[j]);
        if (pathAlive && j >= jmin) {
            spine |= (unsigned long long)code << (2 * nsp);
            if (CbR) spineR |= (unsigned long long)cget(CbR, ((int64_t)1 << j) + (blk >> (dl - j))) << (2 * nsp);   // 3 wherever the mid code is
            ++nsp;
        }
        if (code == 3 && pathAlive) {
            // first pruned node on the path: it is emitted itself, by the block holding ITS first leaf
            alive = ((blk >> (dl - j)) << (dl - j)) == blk;
            pathAlive = false;
        }
    }
    const int64_t o = (int64_t)brick * a.nEmitBlk + blk;
    a.blockAlive[o] = (uint8_t)((alive ? 1 : 0) | (pathAlive ? 2 : 0));   // bit1: the depth-(D-sub) node itself is live
    a.blockVal[o] = (uint8_t)val;            // scalar of the depth-(D-sub-1) parent (codes applied down to depth dl-1)
    a.blockSpine[o] = spine | ((unsigned long long)nsp << 56);
    if (CbR) a.blockSpineR[o] = spineR | ((unsigned long long)nsp << 56);
    // tokens this block emits: the upper spine its first rank owns + its own subtree if that is live
    // (k_prune_emit12 left the subtree's count in blockOff[], which k_emit_scan overwrites afterwards)
    a.blockTot[o] = (uint32_t)nsp + (pathAlive ? a.blockOff[o] : 0u);
}

// The decode index of a fused build: block-local offsets -> offsets into the gapped stream buffer (slot b starts at
// token b * PE_TOKENS), the scalar decoded down to depth Ds, and the scalars of the eight depth-(D-3) nodes below it
// (k_decode_quad).  Codes under a pruned node are all 3, so the walks are the same for live and dead entries.
// This kernel: a wave per block; the `index_per_block` switch launches it, and it is the reference for k_index12 below.
__global__ void __launch_bounds__(256)
k_index12_block(EmitArgs a, uint32_t nblk)
{   // a wave per block, four per workgroup (one-wave workgroups: two million of them were dispatch-bound)
    const int brick = blockIdx.y, t = threadIdx.x & 63, D = a.D;
    Ctrl &c = a.ctrls[brick];
    if (c.constBrick) return;
    const uint32_t blk = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (blk >= nblk) return;
    const int64_t bo = (int64_t)brick * a.nEmitBlk + blk;
    const int bflags = a.blockAlive[bo];
    const int bval = a.blockVal[bo];
    const uint32_t s = (blk << 6) + (uint32_t)t;                        // my depth-Ds (= D-6) subtree
    const int64_t io = (int64_t)brick * a.nIdx + s;
    const uint8_t *Cb = a.codes + (int64_t)brick * a.codeStride;
    {   // a block whose root is a pruned token (two thirds of the bench volume's: constant regions), or that lies under
        // one: every code below moves nothing (3s, or the "keep"s the level loop left under a root k_prune_emit12
        // pruned), so all 64 entries are dead with the scalar above the block -- one byte decides, nothing else is read
        const int64_t nr = ((int64_t)1 << (D - 12)) + blk;
        const uint32_t rootCode = ((uint32_t)Cb[nr >> 2] >> ((int)(nr & 3) * 2)) & 3u;
        if (rootCode == 3u || !(bflags & 2)) {
            a.idxOff[io] = VR_IDX_DEAD;
            if (a.idxBase && t == 0) a.idxBase[bo] = (unsigned long long)blk * PE_TOKENS;
            a.idxVal[io] = (uint8_t)bval;
            *(uint2 *)(a.idxVal3 + io * 8) = make_uint2((uint32_t)bval * 0x01010101u, (uint32_t)bval * 0x01010101u);
            return;
        }
    }
    const uint32_t local = a.idxOff[io];
    uint32_t cb[7];
    int csh[7], dist[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const int j = D - 12 + q;
        const int64_t ni = ((int64_t)1 << j) + (s >> (6 - q));
        cb[q] = Cb[ni >> 2];
        csh[q] = (int)(ni & 3) * 2;
        dist[q] = c.distanceMap[j];
    }
    // the three levels below my node (2 + 4 + 8 codes: the level loop's own, pruning only ever turns a 0 into a 3 and
    // neither moves a scalar) for the depth-(D-3) scalars k_decode_quad starts from
    const int64_t n5 = ((int64_t)1 << (D - 5)) + 2 * (int64_t)s, n4 = ((int64_t)1 << (D - 4)) + 4 * (int64_t)s,
                  n3 = ((int64_t)1 << (D - 3)) + 8 * (int64_t)s;
    const uint32_t c5 = (uint32_t)Cb[n5 >> 2] >> ((int)(n5 & 3) * 2), c4 = Cb[n4 >> 2], c3 = *(const uint16_t *)(Cb + (n3 >> 2));
    const int dl5 = c.distanceMap[D - 5], dl4 = c.distanceMap[D - 4], dl3 = c.distanceMap[D - 3];
    int val = bval;                             // scalar of the block root's parent
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const int code = (int)((cb[q] >> csh[q]) & 3u);
        val = (D - 12 + q) == 0 ? val : apply_code(val, code, dist[q]);
    }
    // (64-bit trees: the entry stays relative to the block, whose slot offset goes to idxBase)
    // an entry whose own token is a 3 is as good as one under a pruned node: all its voxels take its scalar, and a
    // decoder that sees "dead" fills them without touching the stream
    const bool root3 = ((cb[6] >> csh[6]) & 3u) == 3u;
    a.idxOff[io] = ((bflags & 2) && local != VR_IDX_DEAD && !root3) ? (a.idxBase ? 0u : blk * (uint32_t)PE_TOKENS) + local : VR_IDX_DEAD;
    if (a.idxBase && t == 0) a.idxBase[bo] = (unsigned long long)blk * PE_TOKENS;
    a.idxVal[io] = (uint8_t)val;
    uint32_t lo3 = 0, hi3 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int v = apply_code(val, (int)((c5 >> (2 * (i >> 2))) & 3u), dl5);
        v = apply_code(v, (int)((c4 >> (2 * (i >> 1))) & 3u), dl4);
        v = apply_code(v, (int)((c3 >> (2 * i)) & 3u), dl3);
        if (i < 4) lo3 |= (uint32_t)v << (8 * i); else hi3 |= (uint32_t)v << (8 * (i - 4));
    }
    *(uint2 *)(a.idxVal3 + io * 8) = make_uint2(lo3, hi3);
}

// apply_code without branches: + dist for code 1, - dist for code 2, nothing for 0 and 3 (v and dist are bytes, so one
// clamp to 0 .. 255 serves both directions)
__device__ __forceinline__ int idx_step(int v, uint32_t code, int dist)
{
    const int m = (int)(code & 1u) - (int)((code >> 1) & 1u);
    return min(max(v + __mul24(m, dist), 0), 255);
}

// What a lane of k_index12 loads for its entry of a live block: the block-local offset k_prune_emit12 left, the code
// bytes of the six nodes on its path below the block's root (whose code the prologue left in LDS), and the 2 + 4 + 8
// codes below its node.  Raw bytes: the shifts wait for the evaluation, so that nothing waits for a load issued one
// block ahead.
struct IdxLoads {
    uint32_t local, cb[7], c5, c4, c3;      // (cb[0] stays unused)
};

// first node of block blk at depth D-12+q (q = 0 .. 6), and where lane's node of that depth sits from the byte of it
__device__ __forceinline__ uint64_t idx_first(int D, uint32_t blk, int q) { return ((uint64_t)1 << (D - 12 + q)) + ((uint64_t)blk << q); }
__device__ __forceinline__ uint32_t idx_off(uint64_t u, uint32_t lane, int q) { return (uint32_t)(u & 3u) + (lane >> (6 - q)); }

__device__ __forceinline__ IdxLoads idx_loads(const EmitArgs &a, const uint8_t *Cb, int64_t io0, uint32_t blk, uint32_t lane)
{   // blk is wave-uniform: every address is a scalar base and a small lane offset
    IdxLoads L;
    const int D = a.D;
    L.local = a.idxOff[io0 + ((int64_t)blk << 6) + lane];
#pragma unroll
    for (int q = 1; q < 7; ++q) {
        const uint64_t u = idx_first(D, blk, q);
        L.cb[q] = (Cb + (u >> 2))[idx_off(u, lane, q) >> 2];
    }
    // depths D-5, D-4, D-3: 2, 4 and 8 codes per entry, so 4, 8 and 16 bits at fixed places
    L.c5 = (Cb + (((uint64_t)1 << (D - 7)) + ((uint64_t)blk << 5)))[lane >> 1];
    L.c4 = (Cb + (((uint64_t)1 << (D - 6)) + ((uint64_t)blk << 6)))[lane];
    L.c3 = ((const uint16_t *)(Cb + (((uint64_t)1 << (D - 5)) + ((uint64_t)blk << 7))))[lane];
    return L;
}

// The decode index of a fused build, IDX_BLOCKS consecutive 4096-leaf blocks of a brick per workgroup (the same bytes
// as k_index12_block).  Two thirds of the bench volume's blocks are dead -- their root is a pruned token or lies under
// one -- and all their 64 entries are one value: one byte of flags, one of value and the root's code byte decide that,
// loaded for all blocks in one batch by the first lanes.  The blocks' index ranges are contiguous (IDX_BLOCKS * 256
// bytes of idxOff, * 64 of idxVal, * 512 of idxVal3): all 256 threads walk them in aligned 16-byte pieces and store
// those of dead blocks, so a run of dead blocks is whole 128-byte lines.  Live blocks go to a list in LDS; wave w takes
// entries w, w + 4, ... with the next block's loads issued before this one is evaluated; the level distances come from
// LDS, once per workgroup.  The eight depth-(D-3) scalars of an entry are the leaves of one 2 + 4 + 8 tree: 14 steps
// with shared parents.  A constant brick is IDX_BLOCKS dead blocks of its value (idxOff and idxVal only: what
// k_const_finish wrote for it; idxVal3 of such a brick has no reader).
#ifndef IDX_BLOCKS
#define IDX_BLOCKS 32
#endif
static_assert(IDX_BLOCKS == 16 || IDX_BLOCKS == 32 || IDX_BLOCKS == 64, "one lane of the first wave per block; whole pieces per thread");
__global__ void __launch_bounds__(256)
k_index12(EmitArgs a, uint32_t nblk)
{
    __shared__ uint8_t deadS[IDX_BLOCKS], valS[IDX_BLOCKS], rootS[IDX_BLOCKS], listS[IDX_BLOCKS];
    __shared__ uint32_t distS[10], nLiveS;
    const int brick = blockIdx.y, t = threadIdx.x, D = a.D;
    Ctrl &c = a.ctrls[brick];
    const uint32_t blk0 = blockIdx.x * (uint32_t)IDX_BLOCKS;
    const uint32_t nb = nblk - blk0 < (uint32_t)IDX_BLOCKS ? nblk - blk0 : (uint32_t)IDX_BLOCKS;      // D = 12 .. 16: fewer blocks than lanes
    const int64_t io0 = (int64_t)brick * a.nIdx;
    uint4 *const pOff = (uint4 *)(a.idxOff + io0 + ((int64_t)blk0 << 6));
    uint4 *const pVal = (uint4 *)(a.idxVal + io0 + ((int64_t)blk0 << 6));
    uint4 *const pVal3 = (uint4 *)(a.idxVal3 + (io0 + ((int64_t)blk0 << 6)) * 8);
    const uint4 dead4 = make_uint4(VR_IDX_DEAD, VR_IDX_DEAD, VR_IDX_DEAD, VR_IDX_DEAD);
    if (c.constBrick) {
        const uint32_t v4 = (uint32_t)(uint8_t)c.constVal * 0x01010101u;
#pragma unroll
        for (int k = 0; k < IDX_BLOCKS / 16; ++k) {
            const uint32_t p = (uint32_t)t + 256u * k;
            if ((p >> 4) < nb) pOff[p] = dead4;
        }
        if (t < IDX_BLOCKS * 4 && ((uint32_t)t >> 2) < nb) pVal[t] = make_uint4(v4, v4, v4, v4);
        return;
    }
    const uint8_t *Cb = a.codes + (int64_t)brick * a.codeStride;
    // ---- prologue: the blocks' classes and values, the live list, the level distances
    if (t < 64) {
        bool live = false;
        if ((uint32_t)t < nb) {
            const uint32_t blk = blk0 + (uint32_t)t;
            const int64_t bo = (int64_t)brick * a.nEmitBlk + blk;
            const int bflags = a.blockAlive[bo];
            const int bval = a.blockVal[bo];
            const int64_t nr = ((int64_t)1 << (D - 12)) + blk;
            const uint32_t rootCode = ((uint32_t)Cb[nr >> 2] >> ((int)(nr & 3) * 2)) & 3u;
            live = !(rootCode == 3u || !(bflags & 2));
            deadS[t] = live ? 0 : 1;
            valS[t] = (uint8_t)bval;
            rootS[t] = (uint8_t)rootCode;
            if (a.idxBase) a.idxBase[bo] = (unsigned long long)blk * PE_TOKENS;
        }
        const unsigned long long lm = __ballot(live);
        if (live) listS[__popcll(lm & (((unsigned long long)1 << t) - 1ull))] = (uint8_t)t;
        if (t == 0) nLiveS = (uint32_t)__popcll(lm);
    } else if (t < 74)
        distS[t - 64] = c.distanceMap[D - 12 + (t - 64)];       // depths D-12 .. D-3
    __syncthreads();
    const uint32_t nLive = nLiveS;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(t >> 6), lane = (uint32_t)t & 63u;
    IdxLoads cur = {};
    if (w < nLive) cur = idx_loads(a, Cb, io0, blk0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)listS[w]), lane);
    // ---- dead blocks: at most 2 + 1 + 4 pieces per thread
    if (nLive < nb) {
#pragma unroll
        for (int k = 0; k < IDX_BLOCKS / 16; ++k) {
            const uint32_t p = (uint32_t)t + 256u * k, b = p >> 4;
            if (b < nb && deadS[b]) pOff[p] = dead4;
        }
        if (t < IDX_BLOCKS * 4) {
            const uint32_t b = (uint32_t)t >> 2;
            if (b < nb && deadS[b]) { const uint32_t v4 = (uint32_t)valS[b] * 0x01010101u; pVal[t] = make_uint4(v4, v4, v4, v4); }
        }
#pragma unroll
        for (int k = 0; k < IDX_BLOCKS / 8; ++k) {
            const uint32_t p = (uint32_t)t + 256u * k, b = p >> 5;
            if (b < nb && deadS[b]) { const uint32_t v4 = (uint32_t)valS[b] * 0x01010101u; pVal3[p] = make_uint4(v4, v4, v4, v4); }
        }
    }
    if (w >= nLive) return;
    // ---- live blocks
    int dist[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) dist[i] = __builtin_amdgcn_readfirstlane((int)distS[i]);
    if (D == 12) dist[0] = 0;                       // the brick's root has no code to apply: its scalar is the root distance
    const auto entry = [&](const IdxLoads &L, uint32_t b) {
        const uint32_t blk = blk0 + b;
        int val = idx_step(valS[b], rootS[b], dist[0]);         // valS: the scalar of the block root's parent
        uint32_t code6 = 0;
#pragma unroll
        for (int q = 1; q < 7; ++q) {
            code6 = L.cb[q] >> ((idx_off(idx_first(D, blk, q), lane, q) & 3u) * 2u);
            val = idx_step(val, code6, dist[q]);
        }
        const uint32_t c5 = L.c5 >> ((lane & 1u) * 4u);
        // an entry whose own token is a 3 is as good as one under a pruned node (k_index12_block)
        const bool root3 = (code6 & 3u) == 3u;
        const int64_t io = io0 + ((int64_t)blk << 6) + lane;
        a.idxOff[io] = (L.local != VR_IDX_DEAD && !root3) ? (a.idxBase ? 0u : blk * (uint32_t)PE_TOKENS) + L.local : VR_IDX_DEAD;
        a.idxVal[io] = (uint8_t)val;
        // depth D-5: two nodes; D-4: four; D-3: eight -- each parent evaluated once
        int v5[2], v4[4];
        uint32_t lo3 = 0, hi3 = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) v5[i] = idx_step(val, c5 >> (2 * i), dist[7]);
#pragma unroll
        for (int i = 0; i < 4; ++i) v4[i] = idx_step(v5[i >> 1], L.c4 >> (2 * i), dist[8]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t v = (uint32_t)idx_step(v4[i >> 1], L.c3 >> (2 * i), dist[9]);
            if (i < 4) lo3 |= v << (8 * i); else hi3 |= v << (8 * (i - 4));
        }
        *(uint2 *)(a.idxVal3 + io * 8) = make_uint2(lo3, hi3);
    };
    const auto block_of = [&](uint32_t e) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)listS[e]); };
    // two entries per trip, so that the loads of one are in flight while the other is evaluated, without a copy; the
    // loads are unconditional (past the end of the list: the entry at hand again, from L1, evaluated by nobody), so that
    // the wait before an evaluation counts exactly the loads issued after its own
    for (uint32_t e = w; e < nLive; e += 8u) {
        const uint32_t e1 = e + 4u < nLive ? e + 4u : e;
        const IdxLoads oth = idx_loads(a, Cb, io0, blk0 + block_of(e1), lane);
        entry(cur, block_of(e));
        if (e1 == e) break;
        const uint32_t e2 = e + 8u < nLive ? e + 8u : e1;
        cur = idx_loads(a, Cb, io0, blk0 + block_of(e2), lane);
        entry(oth, block_of(e1));
    }
}

// The reference's contiguous layout (R.cpp:631-718 writes one array): block b contributes the upper spine its first rank
// owns (k_block_alive) and, if its depth-(D-12) root is live, its string from the gapped buffer, at token offset
// blockOff[b] of the brick's stream (a.tree / a.treeR = the destination, brick b at a.brickOff[b]).
// A workgroup takes 16 consecutive blocks = one contiguous piece of the stream: their metadata in one batch of loads;
// the short ones (two thirds of the bench volume's blocks are a spine and one token) by one lane each; the long ones
// by all 256 threads, four destination words per thread and trip from five source words (one 16-byte and one 4-byte
// load, funnel shifts, one 16-byte store).  A word two blocks share is merged in LDS and written once; only the
// piece's very first and last word can belong to a neighbouring workgroup too: those were zeroed by k_emit_zero and
// take atomicOr (two atomics per workgroup instead of two per block: the atomics were a third of this kernel).
#define CC_BLOCKS 16
#define CC_BATCH 4          // chunks per thread whose loads are in flight together
template <bool RANGE>        // RANGE: MidRangeTree's second stream -- same offsets and shape, its own strings and spine
__global__ void __launch_bounds__(256)
k_concat12(EmitArgs a, const uint8_t *__restrict__ gap, int64_t nblk)
{
    __shared__ unsigned long long g0S[CC_BLOCKS], spineS[CC_BLOCKS];
    __shared__ uint32_t totS[CC_BLOCKS], cntS[CC_BLOCKS];
    __shared__ unsigned long long bwIdx[2 * CC_BLOCKS];     // boundary words: destination word index (~0: unused slot) ...
    __shared__ uint32_t bwVal[2 * CC_BLOCKS];               // ... and this block's bits of it
    __shared__ uint32_t chunkPre[CC_BLOCKS + 1];            // long blocks: first chunk of every block in the workgroup's chunk list
    __shared__ uint8_t chunkBlk[CC_BLOCKS * (PE_WORDS / 4 + 4)];   // ... and the block of every chunk
    const int brick = blockIdx.y, t = threadIdx.x;
    Ctrl &c = a.ctrls[brick];
    if (c.constBrick) return;
    if (a.brickOff && a.brickOff[gridDim.y] > (unsigned long long)a.compactCap) return;       // (did not fit: the host regrows and repeats)
    const int64_t blk0 = (int64_t)blockIdx.x * CC_BLOCKS;
    const int64_t base = a.brickOff ? (int64_t)a.brickOff[brick] : (int64_t)brick * a.treeCap;
    uint32_t *G0 = (uint32_t *)((RANGE ? a.treeR : a.tree) + base);
    const uint64_t capTok = a.brickOff ? ~0ull >> 2 : (uint64_t)a.treeCap * 4ull;            // tokens the brick's buffer holds
    if (t < 2 * CC_BLOCKS) { bwIdx[t] = ~0ull; bwVal[t] = 0u; }
    if (t < CC_BLOCKS) {
        const int64_t blk = blk0 + t;
        unsigned long long g0 = 0, sp = 0;
        uint32_t tot = 0, cnt = 0;
        if (blk < nblk) {
            const int64_t bo = (int64_t)brick * a.nEmitBlk + blk;
            const int bflags = a.blockAlive[bo];
            sp = RANGE ? a.blockSpineR[bo] : a.blockSpine[bo];
            g0 = a.blockOff64 ? a.blockOff64[bo] : (unsigned long long)a.blockOff[bo];
            tot = (bflags & 1) ? a.blockTot[bo] : 0u;
            cnt = (bflags & 2) && tot ? tot - (uint32_t)(sp >> 56) : 0u;      // tokens of the block's own string
            // never write outside the brick's stream buffer, whatever the counts say (a count/emit mismatch would be a
            // bug; it must surface as a failed parity check, not as a memory fault)
            if (tot && g0 + tot + 32ull > capTok) { atomicMax(&c.emitOverflow, 1); tot = 0; cnt = 0; }
        }
        g0S[t] = g0; spineS[t] = sp; totS[t] = tot; cntS[t] = cnt;
    }
    __syncthreads();
    // ---- short blocks (spine + string of at most 32 tokens): one lane each
    if (t < CC_BLOCKS && totS[t] != 0u && totS[t] <= 32u) {
        const unsigned long long g0 = g0S[t];
        const uint32_t tot = totS[t], cnt = cntS[t];
        const int nsp = (int)(spineS[t] >> 56);
        unsigned long long v = spineS[t] & 0x00FFFFFFFFFFFFFFull;
        if (cnt) {
            const uint32_t *slot = (const uint32_t *)(gap + (int64_t)brick * a.treeCap) + (size_t)(blk0 + t) * PE_WORDS;
            unsigned long long sv = slot[0];
            if (cnt > 16u) sv |= (unsigned long long)slot[1] << 32;
            if (cnt < 32u) sv &= (1ull << (2 * cnt)) - 1ull;
            v |= sv << (2 * nsp);
        }
        const uint32_t sh = (uint32_t)(g0 & 15ull) * 2u;
        const uint64_t w0 = g0 >> 4, wl = (g0 + tot - 1) >> 4;       // first and last word (shared with the neighbours)
        const uint32_t x0 = (uint32_t)(v << sh), x1 = (uint32_t)((v << sh) >> 32), x2 = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
        bwIdx[2 * t] = w0; bwVal[2 * t] = x0;
        if (wl == w0 + 1) { bwIdx[2 * t + 1] = wl; bwVal[2 * t + 1] = x1; }
        else if (wl == w0 + 2) { G0[w0 + 1] = x1; bwIdx[2 * t + 1] = wl; bwVal[2 * t + 1] = x2; }
    }
    // ---- long blocks: their 16-byte destination chunks as ONE list over the workgroup's blocks (a prefix over the
    // blocks' chunk counts, a byte per chunk saying whose it is), four chunks per thread and trip with all their loads
    // issued before the first is used: a thread looping over the blocks one after another had one load in flight and
    // sixteen dependent round trips (2.3 ms for the bench volume's 4.5 GB; the copy itself is 1.6)
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < CC_BLOCKS; ++i) {
            chunkPre[i] = run;
            if (totS[i] > 32u) {
                const uint64_t w0 = g0S[i] >> 4, wl = (g0S[i] + totS[i] - 1) >> 4;
                run += (uint32_t)((wl - (w0 & ~3ull)) / 4 + 1);
            }
        }
        chunkPre[CC_BLOCKS] = run;
    }
    __syncthreads();
    const uint32_t nchunkAll = chunkPre[CC_BLOCKS];
    for (int i = 0; i < CC_BLOCKS; ++i)
        for (uint32_t j = chunkPre[i] + (uint32_t)t; j < chunkPre[i + 1]; j += 256u) chunkBlk[j] = (uint8_t)i;
    __syncthreads();
    const uint32_t *gapW = (const uint32_t *)(gap + (int64_t)brick * a.treeCap) + (size_t)blk0 * PE_WORDS;
    for (uint32_t j0 = (uint32_t)t; j0 < nchunkAll; j0 += 256u * CC_BATCH) {
        uint32_t sv[CC_BATCH][5];
        // -- the loads of up to CC_BATCH chunks
#pragma unroll
        for (int k = 0; k < CC_BATCH; ++k) {
            const uint32_t j = j0 + 256u * (uint32_t)k;
#pragma unroll
            for (int m = 0; m < 5; ++m) sv[k][m] = 0u;
            if (j >= nchunkAll) continue;
            const int i = chunkBlk[j];
            const unsigned long long g0 = g0S[i];
            const uint32_t cnt = cntS[i];
            const int nsp = (int)(spineS[i] >> 56);
            const int nws = (int)((cnt + 15u) >> 4);
            const uint32_t *slot = gapW + (size_t)i * PE_WORDS;
            const uint64_t wA = (g0 >> 4) & ~3ull;
            const long long so = 2ll * ((long long)(16ull * wA) - (long long)g0 - nsp) + 128ll * (long long)(j - chunkPre[i]);
            const int sw = (int)(so >> 5);                                 // (floor division)
            if (cnt && sw >= 0 && sw + 4 < nws) {                          // the common case: five words inside the string
                struct __attribute__((packed, aligned(4))) U4 { uint32_t x, y, z, w; };
                const U4 u = *(const U4 *)(slot + sw);
                sv[k][0] = u.x; sv[k][1] = u.y; sv[k][2] = u.z; sv[k][3] = u.w; sv[k][4] = slot[sw + 4];
            } else {
#pragma unroll
                for (int m = 0; m < 5; ++m) sv[k][m] = (cnt && sw + m >= 0 && sw + m < nws) ? slot[sw + m] : 0u;
            }
        }
        // -- shift, edges, store
#pragma unroll
        for (int k = 0; k < CC_BATCH; ++k) {
            const uint32_t j = j0 + 256u * (uint32_t)k;
            if (j >= nchunkAll) continue;
            const int i = chunkBlk[j];
            const unsigned long long g0 = g0S[i];
            const uint32_t tot = totS[i], cnt = cntS[i];
            const int nsp = (int)(spineS[i] >> 56);
            const unsigned long long spine = spineS[i] & 0x00FFFFFFFFFFFFFFull;
            const uint64_t w0 = g0 >> 4, wl = (g0 + tot - 1) >> 4;
            const uint64_t wA = w0 & ~3ull;                                  // first destination word of chunk 0 (16-byte aligned)
            const uint32_t q = j - chunkPre[i];
            const uint64_t d0 = wA + 4ull * (uint64_t)q;                     // my four destination words d0 .. d0+3
            // bit offset of word d0 in the block's string (negative: in front of it)
            const long long so = 2ll * ((long long)(16ull * wA) - (long long)g0 - nsp) + 128ll * (long long)q;
            const uint32_t shf = (uint32_t)(so & 31ll);
            uint32_t o[4];
            const int tok0 = (int)(so >> 1);                               // string token at bit 0 of word d0
            const bool edge = tok0 < 0 || tok0 + 64 > (int)cnt;            // the chunk touches the string's start or end
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                o[m] = __builtin_amdgcn_alignbit(sv[k][m + 1], sv[k][m], shf);
                if (edge) {
                    const int tokAt = tok0 + 16 * m;
                    if (tokAt + 16 > (int)cnt) {        // the string's last word may carry stale bits behind the last token: cut them
                        const int keep = (int)cnt - tokAt;
                        o[m] = keep <= 0 ? 0u : (keep >= 16 ? o[m] : (o[m] & ((1u << (2 * keep)) - 1u)));
                    }
                    if (tokAt < 0 && nsp) {             // in front of the string: the spine's bits
                        const long long bo2 = 2ll * ((long long)(16ull * (d0 + m)) - (long long)g0);
                        o[m] |= bo2 >= 0 ? (bo2 < 64 ? (uint32_t)(spine >> bo2) : 0u) : (uint32_t)(spine << (-bo2));
                    }
                }
            }
            if (d0 > w0 && d0 + 3 < wl) {
                *(uint4 *)(G0 + d0) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint64_t d = d0 + m;
                    if (d < w0 || d > wl) continue;
                    if (d == w0) { bwIdx[2 * i] = d; bwVal[2 * i] = o[m]; }
                    else if (d == wl) { bwIdx[2 * i + 1] = d; bwVal[2 * i + 1] = o[m]; }
                    else G0[d] = o[m];
                }
            }
        }
    }
    __syncthreads();
    // ---- the boundary words: slots are in stream order, so equal words are neighbours; the first slot of a word writes
    // the OR of all of them
    if (t < 2 * CC_BLOCKS) {
        const unsigned long long w = bwIdx[t];
        if (w != ~0ull) {
            bool first = true;
            uint32_t v = 0;
            unsigned long long wFirst = ~0ull, wLast = 0;
            for (int j = 0; j < 2 * CC_BLOCKS; ++j) {
                const unsigned long long wj = bwIdx[j];
                if (wj == ~0ull) continue;
                if (wFirst == ~0ull) wFirst = wj;
                wLast = wj;
                if (wj == w) { v |= bwVal[j]; if (j < t) first = false; }
            }
            if (first) {
                if (w == wFirst || w == wLast) { if (v) atomicOr(&G0[w], v); }
                else G0[w] = v;
            }
        }
    }
}

__global__ void __launch_bounds__(1024)
k_emit_stats(EmitArgs a, int64_t nblk)
{
    __shared__ unsigned long long sh[16];
    const int brick = blockIdx.x;
    if (a.ctrls[brick].constBrick) return;
    unsigned long long v = 0;
    for (int64_t i = threadIdx.x; i < nblk; i += blockDim.x) v = stat_merge(v, a.blockL1[(int64_t)brick * a.nEmitBlk + i]);
    for (int o = 32; o > 0; o >>= 1) v = stat_merge(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int i = 0; i < 16; ++i) t = stat_merge(t, sh[i]);
        Ctrl &c = a.ctrls[brick];
        c.statL1 = t & ((1ull << 40) - 1ull);
        c.maxErrBefore = (int)((t >> 40) & 255ull);
        c.maxErrAfter = (int)((t >> 48) & 255ull);
    }
}

// Closed form for a brick of one value v (tolerance >= 1, maxEpochs >= 1, D >= 1): the root's
// distance is v (running mean of the single mismatch |0 - v|), its code is "add" (or "keep" for
// v = 0), every other node reproduces its parent exactly (distance 0, code 0) and is pruned, so
// the stream is [1][3][3] (or [3] for v = 0), all statistics are 0 and every decode-index entry
// is "dead" with scalar v.  Identical to what the general path produces (tests compare both with
// the oracle); it just skips ~all work for the constant regions of a volume.
__global__ void __launch_bounds__(256)
k_const_finish(int D, Ctrl *ctrls, uint8_t *tree, int64_t treeCap, uint32_t *idxOff, uint8_t *idxVal, int64_t nIdx,
               const unsigned long long *brickOff = nullptr, int64_t compactCap = 0)
{
    const int brick = blockIdx.y;
    Ctrl &c = ctrls[brick];
    if (!c.constBrick) return;
    if (brickOff && brickOff[gridDim.y] > (unsigned long long)compactCap) return;
    const int v = c.constVal;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int d = 0; d <= D; ++d) c.distanceMap[d] = d == 0 ? (uint8_t)v : 0;
        c.numActive = v ? 3 : 1;
        *(uint32_t *)(tree + (brickOff ? (int64_t)brickOff[brick] : (int64_t)brick * treeCap)) = v ? 0x3Du : 0x03u;
        c.numReverts = 0; c.maxErrBefore = 0; c.maxErrAfter = 0; c.statL1 = 0; c.emitOverflow = 0;
    }
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < nIdx) {
        idxOff[(int64_t)brick * nIdx + s] = VR_IDX_DEAD;
        idxVal[(int64_t)brick * nIdx + s] = (uint8_t)v;
    }
}

// The half-range stream of such a brick (MidRangeTree): every half range is 0, the root's distance 0 and code "keep",
// the shape the mid stream's (M.cpp:864-865): [0][3][3], or [3] where the mid stream is [3]; distanceMap all zero.
__global__ void k_const_finish_range(int D, Ctrl *ctrlsR, uint8_t *treeR, int64_t treeCap, const unsigned long long *brickOff = nullptr,
                                     int64_t compactCap = 0)
{
    Ctrl &c = ctrlsR[blockIdx.x];
    if (threadIdx.x || !c.constBrick) return;
    if (brickOff && brickOff[gridDim.x] > (unsigned long long)compactCap) return;
    const int v = c.constVal;             // the brick's VALUE (k_ctrl_init): decides the shape only
    for (int d = 0; d <= D; ++d) c.distanceMap[d] = 0;
    c.numActive = v ? 3 : 1;
    *(uint32_t *)(treeR + (brickOff ? (int64_t)brickOff[blockIdx.x] : (int64_t)blockIdx.x * treeCap)) = v ? 0x3Cu : 0x03u;
    c.numReverts = 0; c.maxErrBefore = 0; c.maxErrAfter = 0; c.statL1 = 0; c.emitOverflow = 0;
}

// ------------------------------------------------------------ host driver ----
static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

static_assert(PEC_BOXES == VR_PEC_BOXES && IDX_BLOCKS == VR_IDX_BLOCKS && EMIT_RANKS_PER_BLOCK == VR_EMIT_RANKS, "host_plan.cpp sizes the grids");

// The level loop of the bricks [b0, b0 + nb) of a stream (every array of a set is per brick: a sub-range is the same
// launches on offset pointers).  Executes plan and build_level(plan, d): nothing is decided here.
static void compress_stream(BrickSet *bs, const BuildPlan &plan, Stream2 &s0, hipStream_t st, const uint8_t *rootMin,
                            const uint8_t *rootMax, SkipBlocks sk, unsigned long long *blockErr, void *estSumm0, int b0, int nb)
{
    const int D = plan.D, B = nb;
    const int64_t mmStride = plan.rootStride;
    struct { Ctrl *ctrl; uint8_t *temp, *codes; uint8_t *recon[3]; } s;
    s.ctrl = s0.ctrl + b0; s.temp = s0.temp + (int64_t)b0 * bs->heapStride; s.codes = s0.codes + (int64_t)b0 * bs->codeStride;
    for (int i = 0; i < 3; ++i) s.recon[i] = s0.recon[i] + (int64_t)b0 * bs->reconStride;
    blockErr += (int64_t)b0 * bs->nErrBlk;
    const int64_t errPlane = (int64_t)bs->B * bs->nErrBlk;     // the minus / plus planes of the partials (leafless leaf level) lie behind the first
    void *estSumm = (uint32_t *)estSumm0 + (int64_t)b0 * bs->estSummStride * (4 * EST_CAND);
    if (plan.skipBlocks) sk.flag += (int64_t)b0 * sk.nBlk;
    if (plan.constClosedForm) { rootMin += (int64_t)b0 * mmStride; rootMax += (int64_t)b0 * mmStride; }
    ReconBufs rb{{s.recon[0], s.recon[1], s.recon[2]}};
    hipLaunchKernelGGL(k_ctrl_init, dim3(B), dim3(64), 0, st, s.ctrl, rootMin, rootMax, mmStride);
    if (plan.zeroFill) { // the loop never runs: tree.resize() / recon.resize() zero-fill is the result
        for (int i = 0; i < 3; ++i) hipMemsetAsync(s.recon[i], 0, (size_t)B * bs->reconStride, st);
        hipMemsetAsync(s.codes, 0, (size_t)B * bs->codeStride, st);
    }
    for (int d = 0; d <= D; ++d) {
        const BuildLevel L = build_level(plan, d);
        // the constant blocks that are not skipped get the two levels k_pyramid12 did not write, in front of their first reader
        if (L.constLeaves)
            hipLaunchKernelGGL(k_fill_const_leaves, dim3(cdiv(sk.nBlk, 256), B), dim3(256), 0, st, D, s.ctrl, s.temp,
                               bs->heapStride, sk);
        hipLaunchKernelGGL(k_est_head, dim3(B), dim3(64), 0, st, d, plan.maxEpochs, s.ctrl, s.temp, bs->heapStride, rb,
                           bs->reconStride, sk);
        for (int r = 0; r < L.est.rounds; ++r) {
            const EstRound &R = L.est.r[r];
            const EstLaunch &E = L.estL[r];
            hipLaunchKernelGGL(E.quads ? k_est_summ<true> : k_est_summ<false>, dim3(E.gx, B), dim3(256), 0, st, d, R.nc, R.segEnd, E.budget,
                               s.ctrl, s.temp, bs->heapStride, rb, bs->reconStride, (uint32_t *)estSumm, bs->estSummStride, sk);
            hipLaunchKernelGGL(k_est_walk, dim3(B), dim3(64), 0, st, d, plan.maxEpochs, R.nc, R.segEnd, r,
                               r == L.est.rounds - 1 ? 1 : 0, E.budget, s.ctrl, s.temp, bs->heapStride, rb, bs->reconStride,
                               (const uint32_t *)estSumm, bs->estSummStride, sk);
        }
        for (int e = 0; e < plan.maxEpochs; ++e) {
            if (L.fill16)
                hipLaunchKernelGGL(L.sumsOnly ? k_fill16<false> : k_fill16<true>, dim3(L.fillGrid, B), dim3(256), 0, st,
                                   d, plan.maxEpochs, s.ctrl, s.temp, s.codes, bs->heapStride, bs->codeStride, rb, bs->reconStride, blockErr,
                                   bs->nErrBlk, sk, errPlane, L.iters);
            else
                hipLaunchKernelGGL(k_fill, dim3(L.fillGrid, B), dim3(256), 0, st, d, s.ctrl, s.temp,
                                   s.codes, bs->heapStride, bs->codeStride, rb, bs->reconStride, blockErr, bs->nErrBlk);
            hipLaunchKernelGGL(k_control, dim3(B), dim3(64), 0, st, d, plan.maxEpochs, plan.guarded ? 1 : 0, s.ctrl, s.temp,
                               bs->heapStride, rb, bs->reconStride, blockErr, bs->nErrBlk, errPlane, L.sumsOnly ? 1 : 0);
        }
        hipLaunchKernelGGL(k_level_end, dim3(B), dim3(64), 0, st, d, s.ctrl);
    }
}

__global__ void k_fix_chain_distances(int D, int maxDepth, Ctrl *ctrls, Ctrl *ctrlsR)
{
    if (threadIdx.x) return;
    const int add[VR_CHAIN_LEVELS] = {64, 32, 16, 8, 4, 2, 1}; // R.cpp:23,94-97
    for (int dd = D + 1, i = 0; dd <= maxDepth; ++dd, ++i) {
        ctrls[blockIdx.x].distanceMap[dd] = (uint8_t)add[i];
        if (ctrlsR) ctrlsR[blockIdx.x].distanceMap[dd] = (uint8_t)add[i];
    }
}

// VRHIP_SYNC=1: synchronise after every phase and report the first failing one (debug aid)
static bool dbg_sync(hipStream_t st, const char *phase)
{
    static const bool on = getenv("VRHIP_SYNC") != nullptr;
    if (!on) return true;
    hipError_t e = hipStreamSynchronize(st);
    fprintf(stderr, "[vrhip] phase %s: %s\n", phase, hipGetErrorString(e));
    return e == hipSuccess;
}

static void fill_emit_args(BrickSet *bs, EmitArgs &a)
{
    const bool mr = bs->plan.midRange;
    a.codes = bs->mid.codes; a.codesR = mr ? bs->rng.codes : nullptr;
    a.temp = bs->mid.temp; a.tempR = mr ? bs->rng.temp : nullptr;
    a.rb = ReconBufs{{bs->mid.recon[0], bs->mid.recon[1], bs->mid.recon[2]}};
    a.rbR = ReconBufs{{bs->rng.recon[0], bs->rng.recon[1], bs->rng.recon[2]}};
    a.ctrls = bs->mid.ctrl; a.ctrlsR = mr ? bs->rng.ctrl : nullptr;
    a.heapStride = bs->heapStride; a.leafStride = bs->reconStride; a.codeStride = bs->codeStride;
    a.D = bs->D; a.maxDepth = bs->maxDepth; a.tol = kernel_tolerance(*bs); a.Ds = bs->Ds; a.K = bs->K;
    a.blockTot = bs->blockTot; a.blockOff = bs->blockOff; a.nEmitBlk = bs->nEmitBlk;
    a.blockOff64 = bs->blockOff64; a.idxBase = bs->idxBase;
    a.blockL1 = bs->blockL1;
    a.blockAlive = bs->blockAlive; a.blockVal = bs->blockVal; a.blockSpine = bs->blockSpine; a.blockSpineR = bs->blockSpineR;
    a.tree = bs->mid.tree; a.treeR = mr ? bs->rng.tree : nullptr; a.treeCap = bs->treeCap;
    a.brickOff = nullptr; a.compactCap = 0;
    a.idxOff = bs->idxOff; a.idxVal = bs->idxVal; a.idxVal3 = bs->idxVal3; a.nIdx = bs->nIdx;
    a.chainLut = bs->chainLut;
}

// The reference's contiguous stream(s) of a fused build, into bs->mid.treeCompact (and rng.treeCompact): the bricks'
// byte offsets (their streams back to back), the words two blocks share zeroed, then spine + string of every block to
// its place.  At the end of build() (BuildPlan::compact) or when the host first asks for bytes.  The buffers are
// sized from the streams' real lengths: the first build of a set guesses, a stream that does not fit raises
// compactOverflow and writes nothing, and the host (capi.hip contiguous_stream) regrows the buffers and repeats.
// Allocates nothing: capi.hip ensure_compact_buffers comes first.
int compact_launch(BrickSet *bs, hipStream_t st)
{
    const BuildPlan &plan = bs->plan;
    const int D = plan.D, B = plan.B;
    const bool mr = plan.midRange;
    if (!bs->brickOff || !bs->compactOverflow || !bs->mid.treeCompact || (mr && !bs->rng.treeCompact)) return -1;
    EmitArgs a;
    fill_emit_args(bs, a);
    a.tree = bs->mid.treeCompact; a.treeR = mr ? bs->rng.treeCompact : nullptr;
    a.brickOff = bs->brickOff; a.compactCap = bs->compactCap;
    const int64_t nblk = plan.nblk;
    // constant bricks first: their token counts (closed form) are part of the offsets
    hipLaunchKernelGGL(k_brick_offsets, dim3(1), dim3(1024), 0, st, bs->mid.ctrl, B, bs->brickOff, bs->compactCap, bs->compactOverflow);
    hipLaunchKernelGGL(k_emit_zero, dim3(cdiv(nblk, 256), B), dim3(256), 0, st, a, nblk);
    hipLaunchKernelGGL(k_concat12<false>, dim3(cdiv(nblk, CC_BLOCKS), B), dim3(256), 0, st, a, bs->mid.tree, nblk);
    if (mr) hipLaunchKernelGGL(k_concat12<true>, dim3(cdiv(nblk, CC_BLOCKS), B), dim3(256), 0, st, a, bs->rng.tree, nblk);
    // (the closed form's stream word only: its index entries were written when the gapped stream was finished)
    hipLaunchKernelGGL(k_const_finish, dim3(1, B), dim3(64), 0, st, D, bs->mid.ctrl, bs->mid.treeCompact,
                       bs->treeCap, bs->idxOff, bs->idxVal, (int64_t)0, bs->brickOff, bs->compactCap);
    if (mr) hipLaunchKernelGGL(k_const_finish_range, dim3(B), dim3(64), 0, st, D, bs->rng.ctrl, bs->rng.treeCompact, bs->treeCap, bs->brickOff, bs->compactCap);
    bs->compactValid = true;
    return launch_status("compact");
}

// Executes a BuildPlan (host_plan.cpp make_build_plan): every `if` below reads a plan field.  Every buffer, stream and
// event it touches exists (capi.hip vr_brickset_build: the side streams, then the plan, then the buffers, then this).
int encode_launch(BrickSet *bs, const BuildPlan &plan, const uint8_t *vox, hipStream_t st)
{
    const int D = plan.D, B = plan.B;
    const bool mr = plan.midRange;
    hipEventRecord(bs->ev[0], st);
    uint8_t *const flag = plan.skipBlocks ? bs->blockFlag : nullptr, *const flagR = plan.skipBlocks && mr ? bs->blockFlagR : nullptr;
    uint8_t *const tempR = mr ? bs->rng.temp : nullptr;
    // ---- BUILD: pyramid.  Each round leaves the (min, max) of its block roots in one of the two carry arrays; the
    // last one each brick's root's
    int buf = 0;
    if (plan.pyr12) {
        const Pyr12Plan &pp = bs->pyr12;      // (planned at create: host_plan.cpp)
        Pyr12Geom pg{};
        pg.ax = pp.ax; pg.ay = pp.ay; pg.az = pp.az;
        memcpy(pg.sx, pp.sx, sizeof(pg.sx));
        pg.swz = pp.swz; pg.nbx = pp.nbx; pg.nby = pp.nby; pg.lnbx = pp.lnbx; pg.lnby = pp.lnby;
        pg.spread = bs->spread;
        // eight boxes per workgroup where they share their 128-byte lines (no XCD order: the sharers are one workgroup)
        hipLaunchKernelGGL(plan.pyr12Lines ? k_pyramid12_lines : k_pyramid12, dim3(plan.pyr12Grid, B), dim3(256), 0, st, bs->g, pg, vox,
                           bs->mid.temp, bs->heapStride, tempR, bs->mmMin[0], bs->mmMax[0], plan.rootStride, flag, flagR);
        buf = 1;
    }
    for (int r = 0; r < plan.pyrRounds; ++r, buf ^= 1) {
        const PyrRound &R = plan.pyr[r];
        const bool fromVoxels = r == 0 && !plan.pyr12;
        hipLaunchKernelGGL(fromVoxels ? k_pyramid<true> : k_pyramid<false>, dim3(R.blocks, B), dim3(256), 0, st, bs->g, R.dLeaf, R.L, vox,
                           fromVoxels ? nullptr : bs->mmMin[buf ^ 1], fromVoxels ? nullptr : bs->mmMax[buf ^ 1],
                           fromVoxels ? (int64_t)0 : plan.rootStride, bs->mid.temp, bs->heapStride, tempR,
                           bs->mmMin[buf], bs->mmMax[buf], plan.rootStride, fromVoxels && plan.pyrSrcIdx ? bs->srcIdx : nullptr);
    }
    const uint8_t *const rootMinP = bs->mmMin[buf ^ 1], *const rootMaxP = bs->mmMax[buf ^ 1];    // the last round's
    hipEventRecord(bs->ev[1], st);
    dbg_sync(st, "pyramid");
    // ---- COMPRESS
    // constant bricks take the closed form
    const uint8_t *cMin = plan.constClosedForm ? rootMinP : nullptr, *cMax = plan.constClosedForm ? rootMaxP : nullptr;
    const SkipBlocks sk{flag, plan.boxes, D - 2};
    const SkipBlocks skR{flagR, plan.boxes, D - 2};
    // MidRangeTree: the two streams' level loops do not depend on each other (M.cpp:399-544 runs them one after the
    // other): the half-range stream's goes to the set's second stream, so its one-wave-per-brick walkers run beside
    // the mid stream's wide kernels and the other way round
    if (plan.forkRange) {
        hipEventRecord(bs->evFork, st);
        hipStreamWaitEvent(bs->aux, bs->evFork, 0);
        compress_stream(bs, plan, bs->rng, bs->aux, cMin, cMax, skR, bs->blockErrR, bs->estSummR, 0, B);
        hipEventRecord(bs->evJoin, bs->aux);
    }
    // VolumeKdtree: the same trick over ranges of the bricks (vr_brickset_set_concurrency; 2 by default)
    if (plan.parts > 1) hipEventRecord(bs->evFork, st);
    for (int p = 1; p < plan.parts; ++p) {
        hipStreamWaitEvent(bs->auxN[p - 1], bs->evFork, 0);
        compress_stream(bs, plan, bs->mid, bs->auxN[p - 1], cMin, cMax, sk, bs->blockErr, bs->estSumm, plan.range[p], plan.range[p + 1] - plan.range[p]);
        hipEventRecord(bs->evJoinN[p - 1], bs->auxN[p - 1]);
    }
    compress_stream(bs, plan, bs->mid, st, cMin, cMax, sk, bs->blockErr, bs->estSumm, 0, plan.range[1]);
    for (int p = 1; p < plan.parts; ++p) hipStreamWaitEvent(st, bs->evJoinN[p - 1], 0);
    if (plan.forkRange) hipStreamWaitEvent(st, bs->evJoin, 0);
    else if (mr) compress_stream(bs, plan, bs->rng, st, cMin, cMax, skR, bs->blockErr, bs->estSumm, 0, B);
    hipEventRecord(bs->ev[2], st);
    dbg_sync(st, "compress");
    // ---- PRUNE
    hipLaunchKernelGGL(k_chain_lut, dim3(1), dim3(256), 0, st, kernel_tolerance(*bs), bs->maxDepth - D, bs->chainLut);
    ReconBufs rb{{bs->mid.recon[0], bs->mid.recon[1], bs->mid.recon[2]}};
    ReconBufs rbR{{bs->rng.recon[0], bs->rng.recon[1], bs->rng.recon[2]}};
    bs->fineHas.assign((size_t)B, 0);
    fine_has_changed(*bs);
    if (plan.fused) {
        PruneEmitArgs pa;
        pa.sk = sk; pa.skR = skR;
        pa.D = D; pa.tol = kernel_tolerance(*bs); pa.maxDepth = bs->maxDepth; pa.ctrls = bs->mid.ctrl;
        pa.temp = bs->mid.temp; pa.codes = bs->mid.codes;
        pa.heapStride = bs->heapStride; pa.codeStride = bs->codeStride; pa.leafStride = bs->reconStride;
        pa.rb = rb; pa.subTok = bs->blockOff; pa.nEmitBlk = bs->nEmitBlk; pa.blockL1 = bs->blockL1;
        pa.chainLut = bs->chainLut; pa.idxOff = bs->idxOff; pa.nIdx = bs->nIdx;
        // the uniform hint of k_decode_region: no flag of an earlier build survives, whichever kernels serve this one
        if (hipMemsetAsync(bs->boxUniform, 0, (size_t)B * (size_t)plan.boxes * sizeof(uint32_t), st) != hipSuccess) return -1;
        pa.fineIdx = (uint32_t *)bs->fineIdx; pa.boxUniform = bs->boxUniform;
        pa.ctrlsR = mr ? bs->rng.ctrl : nullptr; pa.tempR = tempR; pa.codesR = mr ? bs->rng.codes : nullptr;
        pa.rbR = rbR;
        pa.gap = bs->mid.tree; pa.gapR = mr ? bs->rng.tree : nullptr; pa.treeCap = bs->treeCap;
        const dim3 peGrid(plan.pruneGrid, B);
        // constant blocks of a leafless SkipBlocks build have a closed form (k_prune_emit12_const); the two launches
        // write disjoint blocks, and heap nodes 1 .. 3 of a block, whose bytes neighbours share, only through cset3
        pa.uniformBlocks = plan.uniformBlocks;
        if (plan.uniformBlocks)
            hipLaunchKernelGGL(k_prune_emit12_const, dim3(plan.uniformGrid, B), dim3(256), 0, st, pa);
        hipLaunchKernelGGL((plan.leafless ? k_prune_emit12<false, true> : k_prune_emit12<false, false>), peGrid, dim3(256), 0, st, pa);
        if (mr) hipLaunchKernelGGL((plan.leafless ? k_prune_emit12<true, true> : k_prune_emit12<true, false>), peGrid, dim3(256), 0, st, pa);
        bs->fineHas.assign((size_t)B, 1);
        fine_has_changed(*bs);
    } else
        hipLaunchKernelGGL(k_prune_leaf, dim3(plan.pruneGrid, B), dim3(256), 0, st, D, kernel_tolerance(*bs),
                           bs->mid.ctrl, bs->mid.temp, bs->mid.codes, mr ? bs->rng.codes : nullptr, bs->heapStride,
                           bs->codeStride, rb, bs->reconStride, bs->maxDepth, bs->blockL1, bs->nEmitBlk);
    for (int d = plan.pruneFrom; d >= 0; --d)
        hipLaunchKernelGGL(k_prune_level, dim3(cdiv((int64_t)1 << d, 256), B), dim3(256), 0, st, d, bs->mid.ctrl, bs->mid.codes,
                           mr ? bs->rng.codes : nullptr, bs->codeStride);
    hipLaunchKernelGGL(k_fix_chain_distances, dim3(B), dim3(64), 0, st, D, bs->maxDepth, bs->mid.ctrl,
                       mr ? bs->rng.ctrl : nullptr);
    hipEventRecord(bs->ev[3], st);
    dbg_sync(st, "prune");
    // ---- CONVERT
    EmitArgs a;
    fill_emit_args(bs, a);
    const int64_t nblk = plan.nblk;
    if (plan.fused) hipLaunchKernelGGL(k_block_alive, dim3(cdiv(nblk, 256), B), dim3(256), 0, st, a, nblk, 12);   // + token counts
    else hipLaunchKernelGGL(k_emit_count, dim3((unsigned)nblk, B), dim3(EMIT_RANKS_PER_BLOCK), 0, st, a);
    dbg_sync(st, "block_alive/count");
    hipLaunchKernelGGL(k_emit_scan, dim3(B), dim3(1024), 0, st, a, nblk);
    dbg_sync(st, "emit_scan");
    // fused: the strings stay in their slots of the gapped buffer, the decode index points there (k_index12); the
    // contiguous stream is made when the host asks for it (compact_launch)
    bs->gapped = plan.gapped;
    bs->compactValid = false;
    if (plan.index == VR_INDEX12) hipLaunchKernelGGL(k_index12, dim3(plan.indexGrid, B), dim3(256), 0, st, a, (uint32_t)nblk);
    else if (plan.index == VR_INDEX12_BLOCK) hipLaunchKernelGGL(k_index12_block, dim3(plan.indexGrid, B), dim3(256), 0, st, a, (uint32_t)nblk);
    else {
        hipLaunchKernelGGL(k_emit_zero, dim3(cdiv(nblk, 256), B), dim3(256), 0, st, a, nblk);
        hipLaunchKernelGGL(k_emit_write, dim3(plan.indexGrid, B), dim3(EMIT_RANKS_PER_BLOCK), 0, st, a);
    }
    hipLaunchKernelGGL(k_emit_stats, dim3(B), dim3(1024), 0, st, a, plan.statRecords);
    hipLaunchKernelGGL(k_const_finish, dim3(plan.constFinishGrid, B), dim3(plan.constFinishThreads), 0, st, D, bs->mid.ctrl, bs->mid.tree,
                       bs->treeCap, bs->idxOff, bs->idxVal, plan.constFinishIdx);
    if (mr) hipLaunchKernelGGL(k_const_finish_range, dim3(B), dim3(64), 0, st, D, bs->rng.ctrl, bs->rng.tree, bs->treeCap);
    // the reference's build() ends with the contiguous stream (tree.swap(preorderTree), R.cpp:714-718): so does this one,
    // unless the caller turned it off (vr_brickset_set_compaction): the decoders read the block strings where they are
    if (plan.compact) {
        const int rc = compact_launch(bs, st);
        if (rc != 0) return rc;
    }
    hipEventRecord(bs->ev[4], st);
    dbg_sync(st, "emit_write");
    return launch_status("encode");
}

} // namespace vr
