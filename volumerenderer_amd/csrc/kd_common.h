// kd_common.h -- shared types for the gfx950 kd-tree codec kernels.
//
// Layout conventions (per brick; a brickset holds B bricks back to back):
//  * voxels       X*Y*Z uint8, x fastest (reference R.cpp:4-6).
//  * heap arrays  1-based implicit binary heap: node at depth d with path p
//                 (p = Morton prefix, left = 0) lives at index (1<<d) + p, so every
//                 level starts on a power-of-two boundary.  The reference's 0-based
//                 breadth-first index (R.cpp:176-177) is ours minus one.
//  * leaf rank r  path of a depth-D node = the MSB-first interleave of the voxel's
//                 coordinate bits in the reference's split-axis order (R.cpp:151-159).
#pragma once
#include <hip/hip_runtime.h>
#include "host_plan.h"     // Geom, rank_to_xyz, apply_code, cget, VR_MAX_DEPTH / VR_CHAIN_LEVELS / VR_IDX_DEAD

namespace vr {

// Per-brick gradient-descent state (R.cpp:215-227), lives in device memory.
struct Ctrl {
    double currentDistance, currentError, currentDF, currentStepSize;
    double previousDistance, previousError, previousDF, previousStepSize;
    unsigned long long errMinus, errPlus;   // sum err^2 at current-1 / current+1 (exact integers)
    unsigned long long statL1;              // sum |recon-temp| over leaves after branch growth
    unsigned long long numActive;           // numActiveNodes
    int32_t epoch;
    int32_t active;          // the GD loop of this level is still running
    int32_t fillThisEpoch;   // the next fill kernel must run
    int32_t cur, prev, pendingEqual;   // roles of the two level-recon buffers (see kd_encode.hip)
    int32_t par, ra, rb;     // physical recon buffer indices: parents, level buffers
    int32_t numReverts;
    int32_t maxErrBefore, maxErrAfter;
    int32_t estT;            // estimator: the threshold floor(S / (2C + 1)) where the walk stands; the next round's window lies around it
    int32_t estUp;           // estimator: S / (2C + 1) is in the upper half of [estT, estT + 1) (est_window_base)
    int32_t estQuadFb;       // estimator: segments of this level walked node by node in quad rounds, against the level's budget
    unsigned long long estS; // estimator: exact state where the walk stands
    uint32_t estC;
    int32_t estFallbacks;    // segments the estimator had to walk node by node (diagnostic)
    int32_t estSeg;          // estimator: next segment to verify
    int32_t estDone;         // estimator: level finished
    int32_t emitOverflow;    // emit refused to write past the stream buffer (internal error)
    int32_t constBrick;      // every voxel of the brick has the same value: closed-form result (k_const_finish)
    int32_t constVal;
    // which distance the reconstruction in each of the two level buffers (by role) was filled with, and the codes in
    // memory (every fill overwrites them, a revert does not restore them: SURVEY C-2); k_level_end keeps the finished
    // level's pair, which after the loop is the leaf level's: what a leafless build recomputes the leaves from
    int32_t roleDist[2], codesDist, finalReconDist, finalCodesDist;
    // leaf level of a leafless build: its fills store nothing but error partials, so an epoch at the previous fill's
    // distance -1 / +1 needs no fill at all -- that fill's central-difference sums, kept per 1024-node block, ARE the
    // epoch's partials (k_control replays the reference's in-order double accumulation from them).  altValid: the
    // minus / plus planes hold the sums of the fill at distance altDist; altSel: the coming epoch reads plane 1 / 2
    int32_t altValid, altDist, altSel;
    int32_t zeroRun;         // grown branches that ended on an evaluated "keep" code: the reference would rewrite that
                             // run of zeros to 3s (R.cpp:662-669,686-688).  Provably never happens for tolerance >= 0
                             // (the last distance is 1), so the emitters do not implement the rewrite; they count here
                             // and the tests assert zero (the oracle counts its own firings the same way)
    uint8_t distanceMap[VR_MAX_DEPTH + 8];
};

// integer form of encodeNode (R.cpp:457-502): ties keep > add > sub.
struct Enc { int code, recon, err; };
__host__ __device__ inline Enc encode_node(int t, int p, int d)
{
    int none = p > t ? p - t : t - p;
    int add = p + d > 255 ? 255 : p + d;
    int ae = add > t ? add - t : t - add;
    int sub = p - d < 0 ? 0 : p - d;
    int se = sub > t ? sub - t : t - sub;
    int m = none < ae ? none : ae;
    m = se < m ? se : m;
    Enc e;
    e.err = m;
    if (m == none) { e.code = 0; e.recon = p; }
    else if (m == ae) { e.code = 1; e.recon = add; }
    else { e.code = 2; e.recon = sub; }
    return e;
}

#ifdef __HIPCC__
// Two nodes per VALU instruction (packed 16-bit lanes).  encode_node reduces to
//     pd = |t-p|, up = t>p, h = up ? 255-t : t, x = min(d-pd, h), take = |x| < pd
//     err = min(pd,|x|), code = take ? (up ? 1 : 2) : 0, recon = take ? (up ? t+x : t-x) : p
// (the candidate on the far side of the parent never beats "keep", the clamp only ever shortens
// the step: checked exhaustively over all (t,p,d) in tests/test_oracle_golden.py).
typedef short vr_s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short vr_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ vr_s16x2 pk_s(uint32_t v) { return __builtin_bit_cast(vr_s16x2, v); }
__device__ __forceinline__ uint32_t pk_u(vr_s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ vr_s16x2 pk_mad(vr_s16x2 a, vr_s16x2 b, vr_s16x2 c)
{   // a * b + c per 16-bit lane in one instruction (the compiler prefers shift + add for small constant factors)
    vr_s16x2 r;
    asm("v_pk_mad_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ vr_s16x2 pk_abs(vr_s16x2 x) { return __builtin_elementwise_max(x, (vr_s16x2)(0) - x); }
__device__ __forceinline__ uint32_t pk_sumsq(vr_s16x2 e, uint32_t acc)
{
    return __builtin_amdgcn_udot2(__builtin_bit_cast(vr_u16x2, e), __builtin_bit_cast(vr_u16x2, e), acc, false);
}
struct EncPair { vr_s16x2 T2, P2, pd, h; uint32_t up; };   // up: 0xFFFF per lane where t > p
// the sibling pair (bytes 2*tsel, 2*tsel+1 of tword) and their shared parent (byte psel of pword)
__device__ __forceinline__ EncPair enc_pair(uint32_t tword, int tsel, uint32_t pword, int psel)
{
    EncPair c;
    const uint32_t T2 = __builtin_amdgcn_perm(0, tword, tsel ? 0x0c030c02u : 0x0c010c00u);
    const uint32_t P2 = __builtin_amdgcn_perm(0, pword, 0x0c000c00u | (uint32_t)psel | ((uint32_t)psel << 16));
    c.T2 = pk_s(T2); c.P2 = pk_s(P2);
    const vr_s16x2 diff = c.T2 - c.P2, nd = (vr_s16x2)(0) - diff;
    c.pd = __builtin_elementwise_max(diff, nd);
    c.up = pk_u(nd >> 15);
    c.h = pk_s(T2 ^ (c.up & 0x00FF00FFu));
    return c;
}
__device__ __forceinline__ vr_s16x2 enc_pair_x(const EncPair &c, uint32_t d2)   // d2 = dist * 0x10001
{
    return __builtin_elementwise_min(pk_s(d2) - c.pd, c.h);
}
__device__ __forceinline__ vr_s16x2 enc_pair_err(const EncPair &c, uint32_t d2)
{
    return __builtin_elementwise_min(c.pd, pk_abs(enc_pair_x(c, d2)));
}
// wave64 inclusive scans on the DPP network (row shifts inside 16-lane rows, then the two row
// broadcasts): six VALU instructions instead of six LDS-crossbar shuffles.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t identity, uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROWMASK, 0xf, false);
}
// Inside each 16-lane row only (row shifts, no broadcasts): four independent scans / reductions per wave.
__device__ __forceinline__ uint32_t row_incl_scan_add_dpp(uint32_t v)
{
    v += dpp_u32<0x111, 0xf>(0, v);   // row_shr:1
    v += dpp_u32<0x112, 0xf>(0, v);   // row_shr:2
    v += dpp_u32<0x114, 0xf>(0, v);   // row_shr:4
    v += dpp_u32<0x118, 0xf>(0, v);   // row_shr:8
    return v;
}
__device__ __forceinline__ int row_max_i32_dpp(int v)   // the row's maximum, valid in its lane 15
{
    const uint32_t I = 0x80000000u;
    v = max(v, (int)dpp_u32<0x111, 0xf>(I, (uint32_t)v));
    v = max(v, (int)dpp_u32<0x112, 0xf>(I, (uint32_t)v));
    v = max(v, (int)dpp_u32<0x114, 0xf>(I, (uint32_t)v));
    v = max(v, (int)dpp_u32<0x118, 0xf>(I, (uint32_t)v));
    return v;
}
__device__ __forceinline__ int row_min_i32_dpp(int v)   // the row's minimum, valid in its lane 15
{
    const uint32_t I = 0x7FFFFFFFu;
    v = min(v, (int)dpp_u32<0x111, 0xf>(I, (uint32_t)v));
    v = min(v, (int)dpp_u32<0x112, 0xf>(I, (uint32_t)v));
    v = min(v, (int)dpp_u32<0x114, 0xf>(I, (uint32_t)v));
    v = min(v, (int)dpp_u32<0x118, 0xf>(I, (uint32_t)v));
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan_add_dpp(uint32_t v)
{
    v = row_incl_scan_add_dpp(v);
    v += dpp_u32<0x142, 0xa>(0, v);   // row_bcast:15 into rows 1, 3
    v += dpp_u32<0x143, 0xc>(0, v);   // row_bcast:31 into rows 2, 3
    return v;
}
__device__ __forceinline__ int wave_max_i32_dpp(int v)   // result valid in lane 63 (returned via readlane)
{
    const uint32_t I = 0x80000000u;
    v = row_max_i32_dpp(v);
    v = max(v, (int)dpp_u32<0x142, 0xa>(I, (uint32_t)v));
    v = max(v, (int)dpp_u32<0x143, 0xc>(I, (uint32_t)v));
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_min_i32_dpp(int v)   // result valid in lane 63 (returned via readlane)
{
    const uint32_t I = 0x7FFFFFFFu;
    v = row_min_i32_dpp(v);
    v = min(v, (int)dpp_u32<0x142, 0xa>(I, (uint32_t)v));
    v = min(v, (int)dpp_u32<0x143, 0xc>(I, (uint32_t)v));
    return __builtin_amdgcn_readlane(v, 63);
}

#endif

#ifdef __HIPCC__
// Prune only ever turns a 0 into a 3, so an atomic OR of the two bits is race-free whoever
// shares the byte (the per-brick code array is 4-byte aligned).
__device__ inline void cset3(uint8_t *C, int64_t i)
{
    const int64_t b = i >> 2;
    atomicOr((uint32_t *)(C + (b & ~(int64_t)3)), 3u << ((int)(b & 3) * 8 + (int)(i & 3) * 2));
}
#endif

// launch check used by every host launcher: 0 on success; prints the HIP error when
// VRHIP_DEBUG is set in the environment.
int launch_status(const char *what);

} // namespace vr
