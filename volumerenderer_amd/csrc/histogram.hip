// histogram.hip -- what values a volume holds (vrhip.h "volume histograms"): the 256-bin histogram of every brick of a
// buffer and of the whole buffer (vr_histogram_bricks), of the virtual volume of a level-of-detail pool
// (vr_histogram_pool), and the joint histogram of value and gradient magnitude of a dense volume (vr_histogram2d).
// The three entry points are at the end of the file; vr_window_from_histogram is host arithmetic (host_plan.cpp).
//
// Every count is an integer and exact.  Lanes, waves and workgroups are joined by integer adds only, so no result
// depends on the launch shape, on the number of parts or on the order of the atomics.
//
// ---- one dimension: a streaming read of B V bytes, cut into ITEMS as error_table.hip cuts its own
//   k_hist_bricks        V > H_SMALL_V: one workgroup of 256 threads per item (brick, part); a brick has `parts` parts of
//                        `span` bytes (a multiple of 16, at most H_MAX_SPAN).  Every WAVE counts into a 256-bin table of
//                        its own in LDS (ds_add_u32, no return value); after the item thread t adds the four waves' bin t
//                        and sends it on with one device atomic, none for a count of zero.  The same thread keeps bin t
//                        of the TOTAL in a 64-bit register across the items its workgroup walks and sends it once, when
//                        the workgroup ends: the total costs 256 device atomics per workgroup, not per item.
//   k_hist_bricks_small  V <= H_SMALL_V: one TEAM of G lanes per brick (G = 16, 32 or 64), 256 / G bricks per workgroup,
//                        a table per team; thread t then writes bin t of each of the workgroup's bricks (a brick has
//                        one owner: a plain store into the cleared table).
// Both walk their items with a grid stride.  The pool is k_hist_bricks with the item's base, length and weight taken
// from the cell's table entry, read on the device: a stored voxel counts 1 << (sx + sy + sz) times, and an absent
// cell puts X Y Z into bin 0 without touching the pool.
//
// The data-aware paths (template FAST; vr_debug_set("hist_plain", 1) runs the kernels without them, for the tests to
// compare and for the measurements to price): a naive LDS histogram sends all 64 lanes of every wave to ONE address
// wherever the data is constant -- two thirds of the bench volume's 16^3 boxes -- and the LDS serialises them.  So
//   - a 16-byte vector that the whole wave holds as one value (a ballot of "sixteen equal bytes, equal to the first
//     active lane's" against the active lanes) is added by ONE lane for all of them;
//   - otherwise a vector of sixteen equal bytes adds 16 once, a word of four equal bytes adds 4 once;
//   - otherwise byte by byte.
//
// Overflow: the tables in LDS are 32-bit.  A wave's table takes at most one item, H_MAX_SPAN bytes (the static_assert
// below); a pool item's weighted count is at most X Y Z <= 2^32 - 1 (the entry point's check); a per-brick count is
// at most V <= 2^32 - 1 (likewise).  Totals are 64-bit from the register on.
//
// Alignment (vrhip.h "alignment of caller buffers"): an item starts at any byte.  The lanes peel the bytes up to the
// next 16-byte boundary one by one, read aligned 16-byte vectors, and finish the last bytes one by one.
//
// ---- two dimensions: k_hist2d
// Where the 111 x 256 counters live.  Three candidates:
//   (a) one 32-bit copy per workgroup in LDS: 113,664 bytes, so one workgroup per CU; 1024 threads keep 16 waves there,
//       half of what a CU holds.  Cost of a voxel: one ds_add, whatever its row.  Cost of a workgroup: 28,416 counters
//       cleared and scanned once, device atomics for the non-zero ones only.
//   (b) rows 0 .. R-1 in LDS, device atomics for the rows above: more workgroups per CU, but the price of a voxel then
//       depends on the data -- a noisy volume, or one with many edges, sends every voxel to L2 at the contended-atomic rate;
//   (c) device atomics throughout: that rate for every voxel.
// (a) is what is built: its time does not depend on where the data falls in the table.  The grid is at most one
// workgroup per CU, each walking items with a grid stride, so the clear and the scan are paid once per CU.
// An item is H2_SEG consecutive voxels of one x-row of the own box, taken by one wave.  Where X is a multiple of 4 and
// the volume 4-byte aligned, the five rows a voxel reads are aligned alike: the lanes peel the voxels up to the row's
// next 4-byte boundary one by one, then take four voxels a lane from five aligned 32-bit loads plus the two x
// neighbours beyond the word, and finish the last voxels one by one; any other volume goes a voxel per lane and step,
// seven byte loads each.  The wave-uniform shortcut applies: where every active lane has the same (r, v) -- any
// constant region -- one lane adds for all; a lane whose four voxels share a cell adds 4 once.  32-bit counters: a
// workgroup sends its table on and clears it after H2_FLUSH_ROUNDS rounds of 16 items (the static_assert below), so no
// counter can pass 2^32 - 1.
// Addresses: the entry point admits an own box only if every clamped neighbour of every owned voxel lies inside the
// local volume, so every index formed here is inside [0, dims).
#include "brickset.h"
#include "raymarch.h"
#include <algorithm>

namespace vr {

std::atomic<int> g_histPlain{0};

constexpr int H_THREADS = 256;
constexpr int H_BINS = VR_HIST_BINS;
constexpr int64_t H_SMALL_V = 4096;             // up to here a team of one wave's lanes takes a whole brick
constexpr int H_MAX_TEAMS = 16;                 // teams per workgroup of the small kernel: G >= 16
constexpr int64_t H_MIN_SPAN = 16 * 1024;       // four vectors per lane
constexpr int64_t H_MAX_SPAN = 4 * 1024 * 1024;
constexpr int64_t H_TARGET_ITEMS = 8192;        // 256 CUs x 8 workgroups x 4 rounds
constexpr unsigned H_MAX_GRID = 2048;           // 256 CUs x 8 workgroups: the items beyond are walked with the grid stride
static_assert(H_BINS == 256, "a byte has 256 values");
static_assert(H_MAX_SPAN <= 0xFFFFFFFFll, "a wave's 32-bit table takes one item and cannot overflow");
static_assert(H_SMALL_V <= H_MAX_SPAN, "a team's table takes one small brick");
static_assert(H_THREADS == H_BINS, "thread t owns bin t when a table is sent on");
static_assert(sizeof(vr_pool_entry) == 16, "vr_pool_entry is 16 bytes");

// four equal bytes?
__device__ __forceinline__ bool one_byte(uint32_t x) { return x == __builtin_rotateleft32(x, 8); }

template <bool FAST>
__device__ __forceinline__ void hist_word(uint32_t *tab, uint32_t x, uint32_t w)
{
    if (FAST && one_byte(x)) { atomicAdd(&tab[x & 255u], 4u * w); return; }
    atomicAdd(&tab[x & 255u], w);
    atomicAdd(&tab[(x >> 8) & 255u], w);
    atomicAdd(&tab[(x >> 16) & 255u], w);
    atomicAdd(&tab[x >> 24], w);
}

// WAVE: the table belongs to the whole wave (every active lane of the wave is counting into `tab`)
template <bool FAST, bool WAVE>
__device__ __forceinline__ void hist_vec(uint32_t *tab, const uint4 &v, uint32_t w)
{
    if (FAST) {
        const bool one = v.x == v.y && v.x == v.z && v.x == v.w && one_byte(v.x);
        if (WAVE) {
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)v.x);
            const unsigned long long active = __ballot(1), same = __ballot(one && v.x == first);
            if (same == active) {              // (the same in every active lane: no divergence)
                if ((int)__lane_id() == __ffsll((long long)active) - 1)
                    atomicAdd(&tab[first & 255u], 16u * w * (uint32_t)__popcll(active));
                return;
            }
        }
        if (one) { atomicAdd(&tab[v.x & 255u], 16u * w); return; }
    }
    hist_word<FAST>(tab, v.x, w); hist_word<FAST>(tab, v.y, w); hist_word<FAST>(tab, v.z, w); hist_word<FAST>(tab, v.w, w);
}

// bytes [0, len) of p, shared by `lanes` lanes of which this is `lane`, each counting `w`
template <bool FAST, bool WAVE>
__device__ __forceinline__ void hist_range(uint32_t *tab, const uint8_t *__restrict__ p, int64_t len, int lane, int lanes, uint32_t w)
{
    const int64_t head = std::min<int64_t>(len, (16u - ((uint32_t)(uintptr_t)p & 15u)) & 15u);
    // (single bytes mean single-byte loads: the loop vectoriser must not pair them up at an odd address)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int64_t i = lane; i < head; i += lanes) atomicAdd(&tab[p[i]], w);
    const int64_t nvec = (len - head) >> 4;
    const uint4 *vp = (const uint4 *)(p + head);
    int64_t i = lane;
    for (; i + 3 * (int64_t)lanes < nvec; i += 4 * (int64_t)lanes) {     // four loads in flight per lane
        const uint4 a0 = vp[i], a1 = vp[i + lanes], a2 = vp[i + 2 * lanes], a3 = vp[i + 3 * lanes];
        hist_vec<FAST, WAVE>(tab, a0, w); hist_vec<FAST, WAVE>(tab, a1, w);
        hist_vec<FAST, WAVE>(tab, a2, w); hist_vec<FAST, WAVE>(tab, a3, w);
    }
    for (; i < nvec; i += lanes) hist_vec<FAST, WAVE>(tab, vp[i], w);
#pragma clang loop vectorize(disable) interleave(disable)
    for (int64_t t = head + (nvec << 4) + lane; t < len; t += lanes) atomicAdd(&tab[p[t]], w);
}

// POOL: `table` has one entry per item's "brick" (a grid cell), V = X Y Z of a cell; else brick b at data + b V.
// bricks (B x 256, or null) and total (256, or null) are cleared by the caller on the same stream.
template <bool POOL, bool FAST>
__global__ void __launch_bounds__(H_THREADS)
k_hist_bricks(const uint8_t *__restrict__ data, const vr_pool_entry *__restrict__ table, int64_t B, int64_t V, int64_t span,
              int64_t parts, uint32_t *__restrict__ bricks, unsigned long long *__restrict__ total)
{
    __shared__ uint32_t tab[H_THREADS / 64][H_BINS];
    const int t = (int)threadIdx.x, wave = t >> 6;
    unsigned long long tot = 0;                // bin t of the total, over this workgroup's items
    const int64_t items = B * parts;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        for (int w = 0; w < H_THREADS / 64; ++w) tab[w][t] = 0u;
        __syncthreads();
        const int64_t brick = item / parts, lo = (item - brick * parts) * span;
        const uint8_t *p = data;
        int64_t len = 0;
        uint32_t weight = 1u;
        if (POOL) {
            const vr_pool_entry e = table[brick];
            const uint32_t sh = (uint32_t)e.shift[0] + e.shift[1] + e.shift[2];
            if (e.offset < 0) {                // absent: the pool reads as 0 there
                if (lo == 0 && t == 0) tab[0][0] = (uint32_t)V;
            } else if (sh < 32u) {
                weight = 1u << sh;
                len = std::min<int64_t>(span, (V >> sh) - lo);
                p = data + e.offset + lo;
            }
        } else {
            len = std::min<int64_t>(span, V - lo);
            p = data + brick * V + lo;
        }
        if (len > 0) hist_range<FAST, true>(tab[wave], p, len, t, H_THREADS, weight);
        __syncthreads();
        uint32_t c = 0;
        for (int w = 0; w < H_THREADS / 64; ++w) c += tab[w][t];
        if (c != 0u) {
            if (bricks) atomicAdd(&bricks[brick * H_BINS + t], c);
            tot += c;
        }
        __syncthreads();                       // the tables are cleared for the next item
    }
    if (total && tot != 0ull) atomicAdd(&total[t], tot);
}

// lg: log2 of the team width G (4 .. 6)
template <bool FAST>
__global__ void __launch_bounds__(H_THREADS)
k_hist_bricks_small(const uint8_t *__restrict__ data, int64_t B, int64_t V, int lg, uint32_t *__restrict__ bricks,
                    unsigned long long *__restrict__ total)
{
    __shared__ uint32_t tab[H_MAX_TEAMS][H_BINS];
    const int t = (int)threadIdx.x, G = 1 << lg, lane = t & (G - 1), team = t >> lg, perWg = H_THREADS >> lg;
    unsigned long long tot = 0;
    for (int64_t first = (int64_t)blockIdx.x * perWg; first < B; first += (int64_t)gridDim.x * perWg) {
        for (int k = 0; k < perWg; ++k) tab[k][t] = 0u;
        __syncthreads();
        const int64_t brick = first + team;
        if (brick < B) {
            if (lg == 6) hist_range<FAST, true>(tab[team], data + brick * V, V, lane, G, 1u);
            else hist_range<FAST, false>(tab[team], data + brick * V, V, lane, G, 1u);
        }
        __syncthreads();
        for (int k = 0; k < perWg && first + k < B; ++k) {
            const uint32_t c = tab[k][t];
            if (c != 0u) {
                if (bricks) bricks[(first + k) * H_BINS + t] = c;
                tot += c;
            }
        }
        __syncthreads();
    }
    if (total && tot != 0ull) atomicAdd(&total[t], tot);
}

static void parts_of(int64_t B, int64_t V, int64_t &span, int64_t &parts)
{
    parts = std::min<int64_t>((H_TARGET_ITEMS + B - 1) / B, (V + H_MIN_SPAN - 1) / H_MIN_SPAN);
    parts = std::max<int64_t>(parts, (V + H_MAX_SPAN - 1) / H_MAX_SPAN);
    span = ((V + parts - 1) / parts + 15) & ~(int64_t)15;
    parts = (V + span - 1) / span;             // (rounding the span up may leave fewer)
}

// bricks: B x 256 or null, total: 256 or null, both cleared by the caller on the same stream
static int hist_bricks_launch(const uint8_t *data, int64_t B, int64_t V, uint32_t *bricks, unsigned long long *total, hipStream_t st)
{
    const bool fast = g_histPlain.load() == 0;
    if (V <= H_SMALL_V) {
        const int lg = V <= 1024 ? 4 : (V <= 2048 ? 5 : 6);    // a lane holds up to four vectors
        const int64_t perWg = H_THREADS >> lg;
        const unsigned grid = (unsigned)std::min<int64_t>((B + perWg - 1) / perWg, H_MAX_GRID);
        if (fast) hipLaunchKernelGGL(k_hist_bricks_small<true>, dim3(grid), dim3(H_THREADS), 0, st, data, B, V, lg, bricks, total);
        else hipLaunchKernelGGL(k_hist_bricks_small<false>, dim3(grid), dim3(H_THREADS), 0, st, data, B, V, lg, bricks, total);
    } else {
        int64_t span, parts;
        parts_of(B, V, span, parts);
        const unsigned grid = (unsigned)std::min<int64_t>(B * parts, H_MAX_GRID);
        const vr_pool_entry *none = nullptr;
        if (fast) hipLaunchKernelGGL((k_hist_bricks<false, true>), dim3(grid), dim3(H_THREADS), 0, st, data, none, B, V, span, parts, bricks, total);
        else hipLaunchKernelGGL((k_hist_bricks<false, false>), dim3(grid), dim3(H_THREADS), 0, st, data, none, B, V, span, parts, bricks, total);
    }
    return launch_status("hist_bricks");
}

// V = X Y Z of a cell; the parts are cut for a cell stored at full resolution, a coarser one leaves the later ones empty
static int hist_pool_launch(const uint8_t *pool, const vr_pool_entry *table, int64_t cells, int64_t V, uint32_t *perCell,
                            unsigned long long *total, hipStream_t st)
{
    int64_t span, parts;
    parts_of(cells, V, span, parts);
    const unsigned grid = (unsigned)std::min<int64_t>(cells * parts, H_MAX_GRID);
    if (g_histPlain.load() == 0)
        hipLaunchKernelGGL((k_hist_bricks<true, true>), dim3(grid), dim3(H_THREADS), 0, st, pool, table, cells, V, span, parts, perCell, total);
    else
        hipLaunchKernelGGL((k_hist_bricks<true, false>), dim3(grid), dim3(H_THREADS), 0, st, pool, table, cells, V, span, parts, perCell, total);
    return launch_status("hist_pool");
}

// ---- two dimensions ----------------------------------------------------------------------------------------------------
constexpr int H2_THREADS = 1024, H2_WAVES = H2_THREADS / 64;
constexpr int H2_CELLS = VR_HIST_GRAD_BINS * VR_HIST_BINS;
constexpr int64_t H2_SEG = 4096;                // voxels of an item
constexpr uint32_t H2_FLUSH_ROUNDS = 65535;     // rounds of H2_WAVES items between two flushes of a workgroup's table
constexpr unsigned H2_MAX_GRID = 256;           // one workgroup per CU: the table takes most of a CU's LDS
static_assert((unsigned long long)H2_WAVES * H2_SEG * H2_FLUSH_ROUNDS <= 0xFFFFFFFFull,
              "a workgroup's 32-bit counters cannot overflow between two flushes");
static_assert(((441 * 441 <= 3 * 255 * 255) && (442 * 442 > 3 * 255 * 255)) && (441 >> 2) == VR_HIST_GRAD_BINS - 1,
              "isqrt(3 * 255^2) >> 2 is the last row");
static_assert(H2_CELLS * 4 <= 160 * 1024, "the table fits a CU's LDS");

struct Hist2dBox { int64_t dims[3], G[3], org[3], lo[3], hi[3]; };

// the exact integer square root of s <= 3 * 255^2: a float sqrt, corrected by one step either way
__device__ __forceinline__ int isqrt_exact(int s)
{
    int r = (int)__builtin_sqrtf((float)s);
    if (r * r > s) --r;
    else if ((r + 1) * (r + 1) <= s) ++r;
    return r;
}

__device__ __forceinline__ void flush2d(uint32_t *cnt, unsigned long long *__restrict__ hist)
{
    __syncthreads();
    for (int i = (int)threadIdx.x; i < H2_CELLS; i += H2_THREADS) {
        const uint32_t c = cnt[i];
        if (c != 0u) { atomicAdd(&hist[i], (unsigned long long)c); cnt[i] = 0u; }
    }
    __syncthreads();
}

// one row of the own box as a wave walks it: the row of the voxel and of its four y and z neighbours (local pointers),
// and what an x index needs to be clamped in the global volume and made local
struct Row2d {
    const uint8_t *c, *ym, *yp, *zm, *zp;
    int64_t org, last;                         // vol_origin and G - 1 along x
};

template <bool FAST>
__device__ __forceinline__ void count_cell(uint32_t *cnt, int cell, uint32_t n, int lane)
{
    if (FAST) {
        const int first = __builtin_amdgcn_readfirstlane(cell);
        const unsigned long long active = __ballot(1), same = __ballot(cell == first);
        if (same == active) {                  // (the same in every active lane: no divergence)
            if (lane == __ffsll((long long)active) - 1) atomicAdd(&cnt[first], n * (uint32_t)__popcll(active));
            return;
        }
    }
    atomicAdd(&cnt[cell], n);
}

__device__ __forceinline__ int cell_of(int v, int dx, int dy, int dz)
{
    return (isqrt_exact(dx * dx + dy * dy + dz * dz) >> 2) * H_BINS + v;
}

// the voxel at global x, byte loads only
template <bool FAST>
__device__ __forceinline__ void count_voxel(uint32_t *cnt, const Row2d &r, int64_t x, int lane)
{
    const int64_t lx = x - r.org, lxm = std::max<int64_t>(x - 1, 0) - r.org, lxp = std::min<int64_t>(x + 1, r.last) - r.org;
    count_cell<FAST>(cnt, cell_of(r.c[lx], (int)r.c[lxp] - (int)r.c[lxm], (int)r.yp[lx] - (int)r.ym[lx], (int)r.zp[lx] - (int)r.zm[lx]), 1u, lane);
}

__device__ __forceinline__ int byte_of(uint32_t w, int j) { return (int)((w >> (8 * j)) & 255u); }

// items = rows x segs: row (y, z) of the own box, x fastest in y; hist: 111 x 256, cleared by the caller.
// words: X % 4 == 0 and vol 4-byte aligned, so that the five rows of a voxel are aligned alike: a lane then takes four
// voxels from five aligned 32-bit loads and two bytes (the x neighbours beyond the word); the voxels before the first
// aligned one and after the last whole word, and every voxel of a volume that is not `words`, go byte by byte.
template <bool FAST>
__global__ void __launch_bounds__(H2_THREADS)
k_hist2d(const uint8_t *__restrict__ vol, Hist2dBox a, int64_t items, int64_t segs, int words, unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t cnt[H2_CELLS];
    for (int i = (int)threadIdx.x; i < H2_CELLS; i += H2_THREADS) cnt[i] = 0u;
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int64_t X = a.dims[0], XY = a.dims[0] * a.dims[1], oy = a.hi[1] - a.lo[1];
    uint32_t rounds = 0;
    for (int64_t first = (int64_t)blockIdx.x * H2_WAVES; first < items; first += (int64_t)gridDim.x * H2_WAVES) {
        const int64_t item = first + wave;
        if (item < items) {
            const int64_t row = item / segs, seg = item - row * segs;
            const int64_t zz = row / oy, y = a.lo[1] + (row - zz * oy), z = a.lo[2] + zz;          // global
            // clamped in the global volume, then local: inside [0, dims) by the entry point's check
            const int64_t ly = y - a.org[1], lym = std::max<int64_t>(y - 1, 0) - a.org[1], lyp = std::min<int64_t>(y + 1, a.G[1] - 1) - a.org[1];
            const int64_t lz = z - a.org[2], lzm = std::max<int64_t>(z - 1, 0) - a.org[2], lzp = std::min<int64_t>(z + 1, a.G[2] - 1) - a.org[2];
            Row2d r;
            r.c = vol + lz * XY + ly * X; r.ym = vol + lz * XY + lym * X; r.yp = vol + lz * XY + lyp * X;
            r.zm = vol + lzm * XY + ly * X; r.zp = vol + lzp * XY + ly * X;
            r.org = a.org[0]; r.last = a.G[0] - 1;
            const int64_t x0 = a.lo[0] + seg * H2_SEG, x1 = std::min<int64_t>(x0 + H2_SEG, a.hi[0]);
            // [x0, xa) by bytes, [xa, xb) by words, [xb, x1) by bytes
            int64_t xa = x1, xb = x1;
            if (words) {
                xa = std::min<int64_t>(x1, x0 + ((4 - ((x0 - r.org) & 3)) & 3));
                xb = xa + ((x1 - xa) & ~(int64_t)3);
            }
            for (int64_t x = x0 + lane; x < xa; x += 64) count_voxel<FAST>(cnt, r, x, lane);
            for (int64_t x = xa + 4 * (int64_t)lane; x < xb; x += 4 * 64) {
                const int64_t lx = x - r.org;
                const uint32_t c = *(const uint32_t *)(r.c + lx);
                const uint32_t wym = *(const uint32_t *)(r.ym + lx), wyp = *(const uint32_t *)(r.yp + lx);
                const uint32_t wzm = *(const uint32_t *)(r.zm + lx), wzp = *(const uint32_t *)(r.zp + lx);
                const int left = r.c[std::max<int64_t>(x - 1, 0) - r.org], right = r.c[std::min<int64_t>(x + 4, r.last) - r.org];
                int cell[4], sq[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int xm = j > 0 ? byte_of(c, j - 1) : left, xp = j < 3 ? byte_of(c, j + 1) : right;
                    const int dx = xp - xm, dy = byte_of(wyp, j) - byte_of(wym, j), dz = byte_of(wzp, j) - byte_of(wzm, j);
                    sq[j] = dx * dx + dy * dy + dz * dz;
                }
                // isqrt(s) >> 2 is 0 exactly where s < 16: a wave in a smooth region needs no square root at all
                const bool flat = FAST && __all((sq[0] | sq[1] | sq[2] | sq[3]) < 16);
#pragma unroll
                for (int j = 0; j < 4; ++j) cell[j] = (flat ? 0 : (isqrt_exact(sq[j]) >> 2) * H_BINS) + byte_of(c, j);
                if (FAST && cell[0] == cell[1] && cell[0] == cell[2] && cell[0] == cell[3]) {
                    // four voxels in one cell: one add, and one for the wave where every lane agrees.  (Lanes whose
                    // four differ take the other branch: the ballots below compare the lanes that are here.)
                    count_cell<true>(cnt, cell[0], 4u, lane);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) atomicAdd(&cnt[cell[j]], 1u);
                }
            }
            for (int64_t x = xb + lane; x < x1; x += 64) count_voxel<FAST>(cnt, r, x, lane);
        }
        if (++rounds == H2_FLUSH_ROUNDS) { flush2d(cnt, hist); rounds = 0; }       // (the same in every thread)
    }
    flush2d(cnt, hist);
}

static int hist2d_launch(const uint8_t *vol, const Hist2dBox &box, unsigned long long *hist, hipStream_t st)
{
    const int64_t segs = (box.hi[0] - box.lo[0] + H2_SEG - 1) / H2_SEG;
    const int64_t items = (box.hi[1] - box.lo[1]) * (box.hi[2] - box.lo[2]) * segs;
    const unsigned grid = (unsigned)std::min<int64_t>((items + H2_WAVES - 1) / H2_WAVES, H2_MAX_GRID);
    const int words = box.dims[0] % 4 == 0 && ((uintptr_t)vol & 3u) == 0u;     // the rows of a voxel are aligned alike
    if (g_histPlain.load() == 0) hipLaunchKernelGGL(k_hist2d<true>, dim3(grid), dim3(H2_THREADS), 0, st, vol, box, items, segs, words, hist);
    else hipLaunchKernelGGL(k_hist2d<false>, dim3(grid), dim3(H2_THREADS), 0, st, vol, box, items, segs, words, hist);
    return launch_status("hist2d");
}

static bool have_device()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

// the calls' device tables: `words64` 64-bit counters, then `words32` 32-bit ones, in one allocation of the call's own,
// cleared on the stream; after the launch each part that has a destination is downloaded, the stream synchronised, the
// allocation freed
struct CallTables {
    unsigned long long *d64 = nullptr;
    uint32_t *d32 = nullptr;
    size_t bytes64 = 0, bytes32 = 0;
    hipStream_t st = nullptr;

    vr_status open(size_t words64, size_t words32, void *stream)
    {
        st = (hipStream_t)stream;
        bytes64 = words64 * sizeof(unsigned long long);
        bytes32 = words32 * sizeof(uint32_t);
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes64 + bytes32);
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_NO_DEVICE;
        d64 = (unsigned long long *)p;
        d32 = (uint32_t *)((uint8_t *)p + bytes64);
        if (hipMemsetAsync(p, 0, bytes64 + bytes32, st) != hipSuccess) { hipFree(p); d64 = nullptr; return VR_ERR_NO_DEVICE; }
        return VR_OK;
    }
    vr_status close(int rc, void *host64, void *host32)
    {
        hipError_t e = hipSuccess;
        if (rc == 0 && host64 && bytes64) e = hipMemcpyAsync(host64, d64, bytes64, hipMemcpyDeviceToHost, st);
        if (rc == 0 && e == hipSuccess && host32 && bytes32) e = hipMemcpyAsync(host32, d32, bytes32, hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);
        hipFree(d64);
        return rc != 0 || e != hipSuccess || es != hipSuccess ? VR_ERR_NO_DEVICE : VR_OK;
    }
};

} // namespace vr

using namespace vr;

extern "C" {

vr_status vr_histogram_bricks(const uint8_t *data, int32_t num_bricks, int64_t voxels_per_brick, uint32_t *bricks_host,
                              uint64_t *total_host, void *stream)
{
    if (!data || (!bricks_host && !total_host) || num_bricks < 1 || voxels_per_brick < 1 || voxels_per_brick > 0xFFFFFFFFll)
        return VR_ERR_INVALID;
    if (!have_device()) return VR_ERR_NO_DEVICE;
    CallTables t;
    const vr_status s = t.open(total_host ? H_BINS : 0, bricks_host ? (size_t)num_bricks * H_BINS : 0, stream);
    if (s != VR_OK) return s;
    const int rc = hist_bricks_launch(data, num_bricks, voxels_per_brick, bricks_host ? t.d32 : nullptr,
                                      total_host ? t.d64 : nullptr, t.st);
    return t.close(rc, total_host, bricks_host);
}

vr_status vr_histogram_pool(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3],
                            uint32_t *cells_host, uint64_t *total_host, void *stream)
{
    if (!pool || !table || !bd || !grid || (!cells_host && !total_host)) return VR_ERR_INVALID;
    if (((uintptr_t)table & 15u) != 0) return VR_ERR_INVALID;      // the table contract of every pool reader (vrhip.h)
    int64_t V = 1, cells = 1;
    for (int k = 0; k < 3; ++k) {              // vr_raycast_pool's restrictions
        if (bd[k] <= 0 || (bd[k] & (bd[k] - 1)) != 0 || grid[k] <= 0) return VR_ERR_INVALID;
        if (grid[k] >= (1ll << 31) / bd[k]) return VR_ERR_INVALID;
        V *= bd[k];
        if (V > 0xFFFFFFFFll) return VR_ERR_INVALID;
        cells *= grid[k];
        if (cells >= (1ll << 31)) return VR_ERR_INVALID;
    }
    if (!have_device()) return VR_ERR_NO_DEVICE;
    CallTables t;
    const vr_status s = t.open(total_host ? H_BINS : 0, cells_host ? (size_t)cells * H_BINS : 0, stream);
    if (s != VR_OK) return s;
    const int rc = hist_pool_launch(pool, table, cells, V, cells_host ? t.d32 : nullptr, total_host ? t.d64 : nullptr, t.st);
    return t.close(rc, total_host, cells_host);
}

vr_status vr_histogram2d(const uint8_t *vol, const int64_t dims[3], const int64_t global_dims[3], const int64_t vol_origin[3],
                         const int64_t own_lo[3], const int64_t own_hi[3], uint64_t *hist_host, void *stream)
{
    if (!vol || !dims || !global_dims || !vol_origin || !own_lo || !own_hi || !hist_host) return VR_ERR_INVALID;
    Hist2dBox b;
    for (int k = 0; k < 3; ++k) {
        if (dims[k] <= 0 || dims[k] >= (1ll << 31) || global_dims[k] < 0 || global_dims[k] >= (1ll << 31)) return VR_ERR_INVALID;
        const int64_t G = global_dims[k] ? global_dims[k] : dims[k], o = vol_origin[k], end = o + dims[k];
        if (o < 0 || end > G) return VR_ERR_INVALID;                                   // the local volume lies in the global one
        if (own_lo[k] >= own_hi[k]) return VR_ERR_INVALID;                             // empty
        if (own_lo[k] < o || own_hi[k] > end) return VR_ERR_INVALID;                   // leaves the local volume
        if (std::max<int64_t>(own_lo[k] - 1, 0) < o || std::min<int64_t>(own_hi[k], G - 1) > end - 1)
            return VR_ERR_INVALID;                                                     // a clamped neighbour would
        b.dims[k] = dims[k]; b.G[k] = G; b.org[k] = o; b.lo[k] = own_lo[k]; b.hi[k] = own_hi[k];
    }
    if (!have_device()) return VR_ERR_NO_DEVICE;
    CallTables t;
    const vr_status s = t.open(H2_CELLS, 0, stream);
    if (s != VR_OK) return s;
    return t.close(hist2d_launch(vol, b, t.d64, t.st), hist_host, nullptr);
}

} // extern "C"
