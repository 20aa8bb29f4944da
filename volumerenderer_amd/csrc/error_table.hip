// error_table.hip -- per-brick error between two buffers of B bricks x V bytes (vr_brick_error, vrhip.h): the kernel
// behind vr_measure_error_bricks and vr_brickset_error_table.
//
// A streaming read of 2 B V bytes.  The work is cut into ITEMS, one (brick, part) each:
//   k_brick_error       V > ER_SMALL_V: one workgroup of 256 threads per item; a brick has `parts` parts of `span`
//                       bytes (a multiple of 16, at most ER_MAX_SPAN), enough of them that a few bricks still give
//                       every CU several workgroups;
//   k_brick_error_small V <= ER_SMALL_V: one TEAM of G lanes of a wave per brick (G = 4 .. 64, a power of two: a lane
//                       holds up to four 16-byte vectors), 256 / G bricks per workgroup.
// Both walk the items with a grid stride, so any B and V fit the launch limits.
//
// Every field is an integer and exact.  A lane keeps 32-bit partial sums: it sees at most ER_MAX_SPAN / 256 + 30 bytes
// (the static_assert below), so sum (a-b)^2 stays under 2^32 per lane; across lanes the two sums are carried in 64 bits.
// Lanes, waves and workgroups are joined by integer add and max only, so the result does not depend on the launch
// shape, the number of parts or the order of the atomics.  One set of device-scope atomics per item, and none for
// a value of zero (the table is cleared before the launch).
//
// Alignment (vrhip.h "alignment of caller buffers": no reliance on the hardware's tolerance of misaligned vectors):
// an item's two ranges start at any byte, each on its own.  Where both addresses are equal modulo 16 the lanes peel
// the bytes up to the next 16-byte boundary, read 16-byte vectors from both buffers, and finish the last bytes one
// by one (both 16-byte aligned: no head).  Otherwise no vector can be aligned in both buffers: bytes all the way.
#include "brickset.h"
#include <algorithm>

namespace vr {

constexpr int ER_THREADS = 256;
constexpr int64_t ER_SMALL_V = 4096;             // up to here a team of one wave's lanes takes a whole brick
constexpr int64_t ER_MIN_SPAN = 16 * 1024;       // four vectors per lane and buffer
constexpr int64_t ER_MAX_SPAN = 4 * 1024 * 1024;
constexpr int64_t ER_TARGET_ITEMS = 8192;        // 256 CUs x 8 workgroups x 4 rounds
constexpr unsigned ER_MAX_GRID = 1u << 20;
static_assert((ER_MAX_SPAN / ER_THREADS + 32) * 255 * 255 < (1ll << 32), "a lane's 32-bit sum of squares cannot overflow");
static_assert(ER_SMALL_V <= ER_MAX_SPAN / ER_THREADS, "a team's lane sees no more than a workgroup's");
static_assert(sizeof(vr_brick_error) == 24, "vr_brick_error is 24 bytes");

typedef short er_s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short er_u16x2 __attribute__((ext_vector_type(2)));

struct ErrAcc {
    uint32_t s1 = 0, s2 = 0, nd = 0, mx = 0;   // sum |d|, sum d^2, #(d != 0), max |d| of the bytes taken one by one
    er_u16x2 mx2 = {0, 0};                     // max |d| of the vector path: even bytes | odd bytes
};

__device__ __forceinline__ void acc_byte(ErrAcc &c, uint32_t a, uint32_t b)
{
    const uint32_t d = a > b ? a - b : b - a;
    c.s1 += d; c.s2 += d * d; c.nd += d != 0u; c.mx = d > c.mx ? d : c.mx;
}

// four byte pairs at once: the even and the odd bytes as two pairs of 16-bit lanes
__device__ __forceinline__ void acc_word(ErrAcc &c, uint32_t x, uint32_t y)
{
    const uint32_t M = 0x00FF00FFu;
    const er_s16x2 de = __builtin_bit_cast(er_s16x2, x & M) - __builtin_bit_cast(er_s16x2, y & M);
    const er_s16x2 dq = __builtin_bit_cast(er_s16x2, (x >> 8) & M) - __builtin_bit_cast(er_s16x2, (y >> 8) & M);
    const er_u16x2 ae = __builtin_bit_cast(er_u16x2, __builtin_elementwise_max(de, -de));
    const er_u16x2 ao = __builtin_bit_cast(er_u16x2, __builtin_elementwise_max(dq, -dq));
    c.mx2 = __builtin_elementwise_max(c.mx2, __builtin_elementwise_max(ae, ao));
    const uint32_t d = __builtin_bit_cast(uint32_t, ae) | (__builtin_bit_cast(uint32_t, ao) << 8);   // |a - b| per byte
    c.s1 = __builtin_amdgcn_sad_u8(x, y, c.s1);
    c.s2 = __builtin_amdgcn_udot4(d, d, c.s2, false);
    // bit 7 of every byte of d that is not zero
    c.nd += (uint32_t)__builtin_popcount((((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u);
}

__device__ __forceinline__ void acc_vec(ErrAcc &c, const uint4 &a, const uint4 &b)
{
    acc_word(c, a.x, b.x); acc_word(c, a.y, b.y); acc_word(c, a.z, b.z); acc_word(c, a.w, b.w);
}

// bytes [0, len) of a and b, shared by `lanes` lanes of which this is `lane`
__device__ __forceinline__ void acc_range(ErrAcc &c, const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int64_t len,
                                          int lane, int lanes)
{
    const uint32_t ma = (uint32_t)(uintptr_t)a & 15u, mb = (uint32_t)(uintptr_t)b & 15u;
    int64_t head = len;                        // no common alignment: every byte on its own
    if (ma == mb) head = std::min<int64_t>(len, (16u - ma) & 15u);
    // (single bytes mean single-byte loads: the loop vectoriser must not pair them up at an odd address)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int64_t i = lane; i < head; i += lanes) acc_byte(c, a[i], b[i]);
    const int64_t nvec = (len - head) >> 4;
    const uint4 *va = (const uint4 *)(a + head), *vb = (const uint4 *)(b + head);
    int64_t i = lane;
    for (; i + 3 * (int64_t)lanes < nvec; i += 4 * (int64_t)lanes) {     // eight loads in flight per lane
        const uint4 a0 = va[i], a1 = va[i + lanes], a2 = va[i + 2 * lanes], a3 = va[i + 3 * lanes];
        const uint4 b0 = vb[i], b1 = vb[i + lanes], b2 = vb[i + 2 * lanes], b3 = vb[i + 3 * lanes];
        acc_vec(c, a0, b0); acc_vec(c, a1, b1); acc_vec(c, a2, b2); acc_vec(c, a3, b3);
    }
    for (; i < nvec; i += lanes) acc_vec(c, va[i], vb[i]);
#pragma clang loop vectorize(disable) interleave(disable)
    for (int64_t t = head + (nvec << 4) + lane; t < len; t += lanes) acc_byte(c, a[t], b[t]);
}

struct ErrSum { unsigned long long s1, s2; uint32_t nd, mx; };

// joins the `width` lanes of a team (a power of two, 64 = the wave): every lane of the team ends with the team's sums
__device__ __forceinline__ ErrSum team_sum(const ErrAcc &c, int width)
{
    ErrSum r;
    r.s1 = c.s1; r.s2 = c.s2; r.nd = c.nd;
    const uint32_t me = c.mx2.x, mo = c.mx2.y;
    r.mx = std::max(c.mx, std::max(me, mo));
    for (int o = width >> 1; o > 0; o >>= 1) {
        r.s1 += __shfl_xor(r.s1, o); r.s2 += __shfl_xor(r.s2, o); r.nd += __shfl_xor(r.nd, o);
        r.mx = std::max(r.mx, (uint32_t)__shfl_xor(r.mx, o));
    }
    return r;
}

__device__ __forceinline__ void publish(vr_brick_error *e, const ErrSum &r)
{
    if (r.nd == 0u) return;                    // equal ranges: every field stays at the cleared 0
    atomicAdd((unsigned long long *)&e->sum_abs, r.s1);
    atomicAdd((unsigned long long *)&e->sum_sq, r.s2);
    atomicMax(&e->max_abs, r.mx);
    atomicAdd(&e->num_diff, r.nd);
}

__global__ void __launch_bounds__(ER_THREADS)
k_brick_error(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int64_t B, int64_t V, int64_t span, int64_t parts,
              vr_brick_error *__restrict__ out)
{
    __shared__ ErrSum wsum[ER_THREADS / 64];
    const int64_t items = B * parts;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t brick = item / parts, lo = (item - brick * parts) * span;
        const int64_t len = std::min<int64_t>(span, V - lo), base = brick * V + lo;
        ErrAcc c;
        acc_range(c, a + base, b + base, len, (int)threadIdx.x, ER_THREADS);
        const ErrSum r = team_sum(c, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
            ErrSum t = wsum[0];
            for (int w = 1; w < ER_THREADS / 64; ++w) {
                t.s1 += wsum[w].s1; t.s2 += wsum[w].s2; t.nd += wsum[w].nd; t.mx = std::max(t.mx, wsum[w].mx);
            }
            publish(out + brick, t);
        }
        __syncthreads();                       // wsum is rewritten by the next item
    }
}

// lg: log2 of the team width G
__global__ void __launch_bounds__(ER_THREADS)
k_brick_error_small(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int64_t B, int64_t V, int lg,
                    vr_brick_error *__restrict__ out)
{
    const int G = 1 << lg, lane = (int)threadIdx.x & (G - 1), perWg = ER_THREADS >> lg;
    for (int64_t first = (int64_t)blockIdx.x * perWg; first < B; first += (int64_t)gridDim.x * perWg) {
        const int64_t brick = first + ((int)threadIdx.x >> lg);
        ErrAcc c;
        if (brick < B) acc_range(c, a + brick * V, b + brick * V, V, lane, G);
        const ErrSum r = team_sum(c, G);       // (every lane of the wave takes part in the shuffles)
        if (brick < B && lane == 0) publish(out + brick, r);
    }
}

// out: B entries, cleared by the caller on the same stream
int brick_error_launch(const uint8_t *a, const uint8_t *b, int64_t B, int64_t V, vr_brick_error *out, hipStream_t st)
{
    if (V <= ER_SMALL_V) {
        int lg = 2;                            // G * 16 * 4 >= V, G >= 4
        while (lg < 6 && ((int64_t)64 << lg) < V) ++lg;
        const int64_t perWg = ER_THREADS >> lg;
        const unsigned grid = (unsigned)std::min<int64_t>((B + perWg - 1) / perWg, ER_MAX_GRID);
        hipLaunchKernelGGL(k_brick_error_small, dim3(grid), dim3(ER_THREADS), 0, st, a, b, B, V, lg, out);
    } else {
        int64_t parts = std::min<int64_t>((ER_TARGET_ITEMS + B - 1) / B, (V + ER_MIN_SPAN - 1) / ER_MIN_SPAN);
        parts = std::max<int64_t>(parts, (V + ER_MAX_SPAN - 1) / ER_MAX_SPAN);
        const int64_t span = ((V + parts - 1) / parts + 15) & ~(int64_t)15;
        parts = (V + span - 1) / span;         // (rounding the span up may leave fewer)
        const unsigned grid = (unsigned)std::min<int64_t>(B * parts, ER_MAX_GRID);
        hipLaunchKernelGGL(k_brick_error, dim3(grid), dim3(ER_THREADS), 0, st, a, b, B, V, span, parts, out);
    }
    return launch_status("brick_error");
}

} // namespace vr
