// host_plan.cpp -- see host_plan.h.  Plain C++: nothing here touches a device.
#include "host_plan.h"
#include "../../include/vrhip.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <thread>

namespace vr {

// The split-axis rule of buildRecursive (R.cpp:151-159), the only copy on the host (the general-extent kernels of
// kd_decode.hip walk boxes with their own device split_axis): depth d splits axis d % 3, or the next axis that still
// has more than one voxel.  Halves that extent and returns the axis.
static int next_split(int64_t ext[3], int d)
{
    int sd = d % 3, i = 0;
    while (ext[0] * ext[1] * ext[2] > 1 && ext[sd] == 1) sd = (d + ++i) % 3;
    ext[sd] /= 2;
    return sd;
}

void make_geom(Geom &g, const int64_t dims[3])
{
    memset(&g, 0, sizeof(g));
    g.X = (int32_t)dims[0]; g.Y = (int32_t)dims[1]; g.Z = (int32_t)dims[2];
    g.voxels = dims[0] * dims[1] * dims[2];
    int64_t ext[3] = {dims[0], dims[1], dims[2]};
    for (int k = 0; k < 3; ++k) { int n = 0; while (((int64_t)1 << (n + 1)) <= dims[k]) ++n; g.nb[k] = n; }
    g.D = g.nb[0] + g.nb[1] + g.nb[2];         // R.cpp:26-29 (floor of the logarithms)
    // axis[] / bit[]: the per-depth split axis.  Only meaningful for power-of-two extents, where every node of a
    // depth splits the same axis; general extents go through BrickSet::srcIdx / ownerRank instead.
    for (int d = 0; d < g.D && d < 32; ++d) {
        const int sd = next_split(ext, d);
        int b = 0; while (((int64_t)1 << (b + 1)) <= ext[sd]) ++b;
        g.axis[d] = (uint8_t)sd;
        g.bit[d] = (uint8_t)b;                 // the coordinate bit this split decides
    }
}

std::vector<std::array<int, 3>> split_counts(const int64_t dims[3], int depths)
{
    std::vector<std::array<int, 3>> splits((size_t)depths + 1, std::array<int, 3>{{0, 0, 0}});
    int64_t ext[3] = {dims[0], dims[1], dims[2]};
    for (int d = 0; d < depths; ++d) {
        splits[(size_t)d + 1] = splits[(size_t)d];
        ++splits[(size_t)d + 1][(size_t)next_split(ext, d)];
    }
    return splits;
}

std::vector<uint32_t> make_lut(const Geom &g, int K)
{
    std::vector<uint32_t> lut((size_t)1 << K);
    for (uint32_t lr = 0; lr < (1u << K); ++lr) {      // (the low K rank bits are the K deepest levels)
        int x, y, z;
        rank_to_xyz(g, lr, x, y, z);
        lut[lr] = (uint32_t)x | ((uint32_t)y << 10) | ((uint32_t)z << 20);
    }
    return lut;
}

// rank bits of coordinate v of axis ax
static uint32_t rank_bits(const Geom &g, int ax, int v)
{
    uint32_t r = 0;
    for (int d = 0; d < g.D; ++d) {
        r <<= 1;
        if (g.axis[d] == ax) r |= (uint32_t)(v >> g.bit[d]) & 1u;
    }
    return r;
}

std::vector<uint32_t> make_spread(const Geom &g)
{
    std::vector<uint32_t> sp;
    const int ext[3] = {g.X, g.Y, g.Z};
    for (int ax = 0; ax < 3; ++ax)
        for (int v = 0; v < ext[ax]; ++v) sp.push_back(rank_bits(g, ax, v));
    return sp;
}

// The n deepest triples of split levels repeat one order of the three axes and decide coordinate bits n-1 .. 0 (the
// 8^n leaves below a depth-(D-3n) node are then a cube).  pos[axis]: the axis's place in a triple, 0 = deepest.
static bool deep_triples(const Geom &g, int n, int pos[3])
{
    pos[0] = pos[1] = pos[2] = -1;
    for (int q = 0; q < 3; ++q) pos[g.axis[g.D - 3 + q]] = 2 - q;         // deepest level -> rank bit 0
    if (pos[0] < 0 || pos[1] < 0 || pos[2] < 0) return false;
    for (int d = g.D - 3 * n; d < g.D; ++d)
        if (g.axis[d] != g.axis[g.D - 3 + (d - g.D + 3 * n) % 3] || g.bit[d] != (g.D - 1 - d) / 3) return false;
    return true;
}

// k_decode_tile and the kernels built on it (their requirements: the comment above TileArgs, kd_decode.hip)
static bool tile_plan(const Geom &g, int K, TilePlan &a)
{
    if (K != 6 || g.D < 6 || g.X < 128 || g.Y < 8 || g.Z < 4) return false;
    int pos[3];
    if (!deep_triples(g, 2, pos)) return false;
    a.jx = pos[0]; a.jy = pos[1]; a.jz = pos[2];
    a.tilesX = g.X / 128; a.tilesY = g.Y / 8; a.tilesZ = g.Z / 4;
    a.ltx = g.nb[0] - 7; a.lty = g.nb[1] - 3;       // (power-of-two extents: general ones never get here)
    // ticket order inside a group of 256 tiles (k_decode_quad): first the bits that stay inside a 16 x 16 (y, z) cell --
    // z bits 0-1 and y bit 0 of the tile coordinate -- then the others in address order
    const int first[3] = {a.ltx + a.lty, a.ltx + a.lty + 1, a.ltx};
    int n = 0;
    bool used[8] = {};
    for (int i = 0; i < 3; ++i) {
        const bool exists = i < 2 ? (1 << (i + 1)) <= a.tilesZ : a.tilesY >= 2;
        if (exists && first[i] < 8 && !used[first[i]]) { a.kqBit[n++] = (uint8_t)first[i]; used[first[i]] = true; }
    }
    for (int b = 0; b < 8; ++b) if (!used[b]) a.kqBit[n++] = (uint8_t)b;
    return true;
}

// k_decode_region's geometry: the twelve deepest levels must be four (a, b, c) triples in one axis order, deciding
// coordinate bits 3, 2, 1, 0 (a 4096-leaf emit block is then a 16 x 16 x 16 box), with whole 128 x 16 x 16 regions
static bool region_plan(const Geom &g, int K, bool generalGeom, bool idx64, int64_t treeCap, RegionPlan &a)     // a: zeroed
{
    const int D = g.D;
    if (K != 6 || D < 12 || generalGeom || idx64 || (treeCap & 15)) return false;
    if (g.X < VR_RG_REGX || g.X < 128 || g.Y < 16 || g.Z < 16) return false;
    if ((g.X & (g.X - 1)) || (g.Y & (g.Y - 1)) || (g.Z & (g.Z - 1))) return false;
    int pos[3];
    if (!deep_triples(g, 4, pos)) return false;
    const int jx = pos[0], jy = pos[1], jz = pos[2];
    // quad index q = leaf rank >> 2 (10 bits).  Bits 0-5 go to lane / image-word bits: the two lowest x bits first
    int Pmap[6], nx = 0, nxt = 2;
    bool isx[6] = {};
    for (int k = 0; k < 4; ++k) {
        const int qb = 3 * k + jx - 2;
        if (qb >= 0 && qb < 6) { isx[qb] = true; Pmap[qb] = nx++; }
    }
    if (nx != 2) return false;
    for (int qb = 0; qb < 6; ++qb) if (!isx[qb]) Pmap[qb] = nxt++;
    for (int qb = 0; qb < 6; ++qb) a.lanePos |= (uint32_t)qb << (4 * Pmap[qb]);
    const auto word = [&](int q) { uint32_t w = 0; for (int i = 0; i < 6; ++i) if ((q >> i) & 1) w |= 1u << Pmap[i]; return w; };
    for (int gg = 0; gg < 16; ++gg) a.parkP[gg >> 2] |= word(gg) << (8 * (gg & 3));
    for (int sv = 0; sv < 4; ++sv) a.parkS |= word(sv << 4) << (8 * sv);
    // image-word contribution of quad-index bit qb (XOR-linear: a permutation plus the step swizzle)
    const auto contrib = [&](int qb) -> uint32_t {
        if (qb < 6) return 1u << Pmap[qb];
        const int i = qb - 6;
        return (1u << (6 + i)) | (i < 3 ? 1u << (2 + i) : 0u);
    };
    // the eight (y, z) bits of a region's 16 x 16 plane
    struct GB { uint32_t addr, byte, out; } bits[8], ord[8];
    for (int ax = 1; ax <= 2; ++ax)
        for (int k = 0; k < 4; ++k) {
            const int rb = 3 * k + (ax == 1 ? jy : jz);
            GB &b = bits[(ax - 1) * 4 + k];
            b.addr = rb < 2 ? 0u : contrib(rb - 2);
            b.byte = rb < 2 ? 1u << rb : 0u;
            b.out = ax == 1 ? (uint32_t)((1 << k) * g.X) : (uint32_t)((int64_t)(1 << k) * g.X * g.Y);
        }
    // gather bits 0 .. 5-RG_LW come from lane >> RG_LW.  Eight emit blocks per region: bit 1 the plane bit at image bit 5
    // (the 16-byte bank slot's top bit), bits 0 and 2 plane bits that do not move the slot at all (byte index, image bit
    // 9): the eight rows of a store instruction then read conflict-free (the lanes of one row are the eight emit blocks,
    // 4 words = one slot apart).  Four blocks per region: the same three first, any fourth (a two-way conflict at worst).
    bool used[8] = {};
    int n = 0;
    const auto take = [&](int i) { ord[n++] = bits[i]; used[i] = true; };
    int free0 = -1, free1 = -1, top = -1;
    for (int i = 0; i < 8; ++i) {
        if (bits[i].addr == 32u && top < 0) top = i;
        else if ((bits[i].addr & 0x3Cu) == 0u) { if (free0 < 0) free0 = i; else if (free1 < 0) free1 = i; }
    }
    if (free0 >= 0) take(free0); else { for (int i = 0; i < 8; ++i) if (!used[i] && i != top && i != free1) { take(i); break; } }
    if (top >= 0) take(top); else { for (int i = 0; i < 8; ++i) if (!used[i] && i != free1) { take(i); break; } }
    if (free1 >= 0) take(free1); else { for (int i = 0; i < 8; ++i) if (!used[i]) { take(i); break; } }
    for (int i = 0; i < 8; ++i) if (!used[i]) take(i);
    for (int i = 0; i < 8; ++i) {
        a.gAddr[i >> 1] |= ord[i].addr << (16 * (i & 1));
        a.gByte |= ord[i].byte << (4 * i);
        a.gOut[i] = ord[i].out;
    }
    // x bits above the two lowest: the gather's reads
    uint32_t xr[4] = {0, 0, 0, 0};
    if (jx < 2) xr[1] = contrib(3 * 3 + jx - 2);
    else { xr[1] = contrib(6); xr[2] = contrib(9); xr[3] = xr[1] ^ xr[2]; }
    a.xRead[0] = xr[0] | (xr[1] << 16);
    a.xRead[1] = xr[2] | (xr[3] << 16);
    a.jx = jx;
    a.X = g.X; a.Y = g.Y; a.voxels = g.voxels;
    a.lrx = g.nb[0] - 7; a.lry = g.nb[1] - 4;
    a.nreg = (g.X / VR_RG_REGX) * (g.Y / 16) * (g.Z / 16);
    // the emit block of a 16^3 box: the rank bits above the twelve lowest
    uint32_t bpos[3] = {0, 0, 0};
    for (int d = 0; d < D - 12; ++d) {
        const int ax = g.axis[d], kb = g.bit[d] - 4;       // coordinate bit kb + 4 of axis ax sits at rank bit D - 1 - d
        if (kb < 0 || kb >= 6) return false;
        bpos[ax] |= (uint32_t)(D - 1 - d - 12) << (5 * kb);
    }
    a.blkX = bpos[0]; a.blkY = bpos[1]; a.blkZ = bpos[2];
    return true;
}

// k_pyramid12 builds the bottom twelve levels where they split x four times or more (Pyr12Plan::use12)
static bool pyr12_plan(const Geom &g, bool generalGeom, Pyr12Plan &pg)
{
    const int D = g.D;
    if (D < 12 || generalGeom) return false;
    int n[3] = {0, 0, 0};
    for (int q = 0; q < 12; ++q) ++n[g.axis[D - 12 + q]];
    if (n[0] < 4) return false;
    pg.ax = n[0]; pg.ay = n[1]; pg.az = n[2];
    for (int i = 0; i < 16; ++i) pg.sx[i] = (uint16_t)(rank_bits(g, 0, i) & 0xFFFu);   // of x = i, the twelve deepest levels
    const int64_t Bx = g.X >> pg.ax, By = g.Y >> pg.ay, Bz = g.Z >> pg.az;
    const int64_t perLine = (g.X < 128 ? g.X : 128) >> pg.ax;
    pg.swz = (perLine == 8 && Bx % 8 == 0 && ((Bx / 8) * By * Bz) % 8 == 0) ? 1 : 0;
    pg.nbx = (int)Bx; pg.nby = (int)By;
    pg.lnbx = g.nb[0] - pg.ax; pg.lnby = g.nb[1] - pg.ay;
    pg.lines = pg.ax == 4 && g.X >= 128;               // (then nbx % 8 == 0: the extents are powers of two)
    return true;
}

void make_plans(const Geom &g, int K, bool generalGeom, bool idx64, int64_t treeCap, TilePlan &tile, RegionPlan &region,
                Pyr12Plan &pyr12)
{
    tile = TilePlan(); region = RegionPlan(); pyr12 = Pyr12Plan();
    tile.ok = !generalGeom && tile_plan(g, K, tile);
    region.ok = region_plan(g, K, generalGeom, idx64, treeCap, region);
    pyr12.use12 = pyr12_plan(g, generalGeom, pyr12);
}

// a node pruned at depth j stands for every node below it: its value for its descendants at depth L
static void fill_below(std::vector<uint8_t> &v, int L, int j, uint32_t path, int val)
{
    if (j < L) std::fill(v.begin() + ((size_t)path << (L - j)), v.begin() + (((size_t)path + 1) << (L - j)), (uint8_t)val);
}

int cut_values_from_stream(int D, int Ds, int, int64_t nIdx, const uint8_t *tree, int64_t numActive, const uint8_t *dmap,
                           int cut, std::vector<uint8_t> &vals)
{
    vals.assign((size_t)nIdx, 0);
    return walk_stream(D, tree, numActive, dmap, cut,
        [&](int j, uint32_t path, int64_t, int, int val) { if (j == Ds) vals[path] = (uint8_t)val; },
        [&](int j, uint32_t path, int val) { fill_below(vals, Ds, j, path, val); },
        [](uint32_t) {});
}

int build_index_from_stream(int D, int Ds, int K, int64_t nIdx, const uint8_t *tree, int64_t numActive,
                            const uint8_t *dmap, std::vector<uint32_t> &offs, std::vector<uint8_t> &vals,
                            std::vector<uint8_t> &fine, std::vector<uint8_t> &val3)
{
    offs.assign((size_t)nIdx, VR_IDX_DEAD);
    vals.assign((size_t)nIdx, 0);
    // K == 6: tokens owned by each 4-leaf subtree of a depth-Ds node, what k_prune_emit12 leaves for k_decode_fine.
    // A token at depth >= Ds belongs to the 4-leaf subtree that holds its node's first leaf.
    const bool wantFine = K == 6 && D >= 6;
    fine.assign(wantFine ? (size_t)nIdx * 16 : 0, 0);
    val3.assign(wantFine ? (size_t)nIdx * 8 : 0, 0);      // decoded scalar of every depth-(D-3) node (k_decode_quad)
    const auto own = [&](uint32_t path, int j) {
        if (!wantFine || j < Ds) return;
        const uint32_t first = path << (D - j);     // first leaf (rank) below the node
        fine[(size_t)(first >> 6) * 16 + ((first >> 2) & 15u)] += 1;
    };
    return walk_stream(D, tree, numActive, dmap, D,
        [&](int j, uint32_t path, int64_t pos, int, int val) {
            if (j == Ds) { offs[path] = (uint32_t)pos; vals[path] = (uint8_t)val; }
            if (wantFine && j == D - 3) val3[path] = (uint8_t)val;
            own(path, j);
        },
        [&](int j, uint32_t path, int val) {
            fill_below(vals, Ds, j, path, val);     // (the offsets below it stay VR_IDX_DEAD)
            if (wantFine) fill_below(val3, D - 3, j, path, val);
        },
        [&](uint32_t path) { own(path, D); });
}

// ---- block tables ----
int block_table_from_stream(int D, const uint8_t *tree, int64_t numActive, const uint8_t *dmap, uint32_t *blockOff,
                            uint8_t *topVal)
{
    const int Dc = block_depth(D);
    std::fill(blockOff, blockOff + ((size_t)1 << Dc), VR_IDX_DEAD);
    std::fill(topVal, topVal + ((size_t)2 << Dc), (uint8_t)0);
    return walk_stream(D, tree, numActive, dmap, Dc,
        [&](int j, uint32_t path, int64_t pos, int, int val) {
            if (j <= Dc) topVal[((size_t)1 << j) + path] = (uint8_t)val;
            if (j == Dc) blockOff[path] = (uint32_t)pos;
        },
        [&](int j, uint32_t path, int val) {
            for (int L = j + 1; L <= Dc; ++L)
                std::fill(topVal + ((size_t)1 << L) + ((size_t)path << (L - j)), topVal + ((size_t)1 << L) + (((size_t)path + 1) << (L - j)), (uint8_t)val);
        },
        [](uint32_t) {});
}

bool block_table_ok(int D, int64_t numActive, const uint32_t *blockOff)
{
    const int Dc = block_depth(D);
    const int64_t nBlk = (int64_t)1 << Dc;
    if (numActive <= 0 || numActive >= ((int64_t)1 << 32)) return false;
    if (Dc == 0) return blockOff[0] == 0u;
    if (blockOff[0] != VR_IDX_DEAD && blockOff[0] != (uint32_t)Dc) return false;
    int64_t last = -1;
    for (int64_t p = 0; p < nBlk; ++p) {
        if (blockOff[p] == VR_IDX_DEAD) continue;
        // block p's root comes after its Dc ancestors at the least, and after every live block before it
        if ((int64_t)blockOff[p] >= numActive || (int64_t)blockOff[p] <= last || blockOff[p] < (uint32_t)Dc) return false;
        last = blockOff[p];
    }
    return true;
}

// ---- installing streams ----
StreamCheck check_stream(int maxDepth, int64_t treeCap, const vr_tree_desc &d)
{
    if (!d.tree || !d.distance_map || (d.block_off == nullptr) != (d.top_val == nullptr)) return {VR_ERR_INVALID, 0, 0};
    if (d.map_len < maxDepth + 1 || d.num_active <= 0) return {VR_ERR_INVALID, 0, 0};
    if (d.num_active >= (1ll << 32)) return {VR_ERR_UNSUPPORTED, 0, 0};    // token offsets of an installed stream are 32-bit
    const int64_t need = (d.num_active + 3) / 4;
    if (d.tree_bytes < need || need > treeCap) return {VR_ERR_FORMAT, 0, 0};
    return {VR_OK, need, std::min<int64_t>(VR_TREE_TAIL, treeCap - need)};
}

InstallPlan make_install_plan(const InstallInputs &in)
{
    InstallPlan p{};
    const bool device = in.engine == InstallEngine::DEVICE_INDEX;
    const bool beside = in.built && !in.foreign;    // streams are installed into a fresh set, not beside built trees
    p.firstInstall = !in.built;
    p.nBlk = (int64_t)1 << block_depth(in.D);
    p.wantFine = in.K == 6 && in.D >= 6;
    const auto refuse = [&](int status) { p.status = status; p.brick.clear(); return p; };
    if (!in.bricks || !in.descs || in.count < 1 || in.count > in.B) return refuse(VR_ERR_INVALID);
    if (device && (in.variant == VR_VARIANT_MIDRANGE || in.idx64)) return refuse(VR_ERR_UNSUPPORTED);
    if (device && beside) return refuse(VR_ERR_STATE);
    std::vector<uint8_t> named((size_t)in.B, 0);
    bool anyFine = false;
    for (int i = 0; i < in.count; ++i) {
        const int32_t br = in.bricks[i];
        if (br < 0 || br >= in.B || named[(size_t)br]) return refuse(VR_ERR_INVALID);
        named[(size_t)br] = 1;
        const vr_tree_desc &d = in.descs[i];
        const StreamCheck c = check_stream(in.maxDepth, in.treeCap, d);
        if (beside && (c.status == VR_OK || c.status == VR_ERR_FORMAT)) return refuse(VR_ERR_STATE);
        if (c.status != VR_OK) return refuse(c.status);
        const bool fineOk = p.wantFine && std_chain_distances(d.distance_map, in.D);
        anyFine = anyFine || fineOk;
        p.brick.push_back({c.need, c.tail, fineOk,
                           !device ? HostPass::BUILD_INDEX : (d.block_off ? HostPass::TABLE_CHECK : HostPass::TABLE_FROM_STREAM)});
    }
    // the host parse uploads side-cars only where it made them; the kernels write them wherever the geometry has them
    p.needs.idxTop = p.needs.instOff = p.needs.instFlag = p.needs.instList = device;
    p.needs.fineIdx = p.needs.idxVal3 = device ? p.wantFine : anyFine;
    p.needs.idxBase = !device && in.idx64;      // absolute 32-bit offsets from the host parse: the bases are zero
    return p;
}

// ---- the brick-set archive ----
static const char ARCHIVE_MAGIC[8] = {'V', 'R', 'B', 'S', 'E', 'T', '\r', '\n'};
struct ArchiveHeader { char magic[8]; uint32_t version, variant; int64_t dims[3]; int32_t numBricks, D, maxDepth; uint32_t zero; int64_t fileBytes; };
static_assert(sizeof(ArchiveHeader) == VR_ARCHIVE_HEADER_BYTES, "the header is written as it lies in memory");

static int64_t pad16(int64_t n) { return (n + 15) & ~(int64_t)15; }

uint64_t fnv1a64(const uint8_t *p, int64_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (int64_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

void parallel_for(int n, const std::function<void(int)> &fn)
{
    const int workers = std::min(n, 16);
    if (workers <= 1) { for (int i = 0; i < n; ++i) fn(i); return; }
    std::atomic<int> next(0);
    const auto run = [&]() { for (int i = next++; i < n; i = next++) fn(i); };
    std::vector<std::thread> pool;
    for (int w = 1; w < workers; ++w) pool.emplace_back(run);
    run();
    for (auto &t : pool) t.join();
}

int64_t archive_record_bytes(int D, int maxDepth, int64_t treeBytes)
{
    const int Dc = block_depth(D);
    return pad16(maxDepth + 1) + pad16((int64_t)2 << Dc) + pad16((int64_t)4 << Dc) + pad16(treeBytes);
}

ArchiveRecord archive_record(const void *blob, const ArchiveGeom &g, const ArchiveEntry &e)
{
    const int Dc = block_depth(g.D);
    const uint8_t *p = (const uint8_t *)blob + e.offset;
    ArchiveRecord r;
    r.dmap = p; p += pad16(g.maxDepth + 1);
    r.topVal = p; p += pad16((int64_t)2 << Dc);
    r.blockOff = (const uint32_t *)p; p += pad16((int64_t)4 << Dc);
    r.tree = p;
    return r;
}

int archive_parse(const void *blob, int64_t bytes, ArchiveGeom &g, std::vector<ArchiveEntry> &dir)
{
    if (!blob || ((uintptr_t)blob & 3) || bytes < VR_ARCHIVE_HEADER_BYTES) return -1;
    ArchiveHeader h;
    memcpy(&h, blob, sizeof(h));
    if (memcmp(h.magic, ARCHIVE_MAGIC, 8) != 0 || h.version != 1u || h.fileBytes != bytes) return -1;
    if (h.numBricks < 1 || h.D < 0 || h.D > 31 || h.maxDepth != h.D + VR_CHAIN_LEVELS) return -1;
    for (int k = 0; k < 3; ++k) if (h.dims[k] < 1 || h.dims[k] > ((int64_t)1 << 20)) return -1;
    const int64_t dirEnd = VR_ARCHIVE_HEADER_BYTES + (int64_t)h.numBricks * VR_ARCHIVE_ENTRY_BYTES;
    if (dirEnd > bytes) return -1;
    g.variant = (int32_t)h.variant; g.numBricks = h.numBricks; g.D = h.D; g.maxDepth = h.maxDepth;
    for (int k = 0; k < 3; ++k) g.dims[k] = h.dims[k];
    dir.resize((size_t)h.numBricks);
    memcpy(dir.data(), (const uint8_t *)blob + VR_ARCHIVE_HEADER_BYTES, (size_t)h.numBricks * VR_ARCHIVE_ENTRY_BYTES);
    for (const ArchiveEntry &e : dir) {
        if (e.offset == 0) continue;
        if (e.offset < dirEnd || (e.offset & 15) || e.numActive <= 0 || e.numActive >= ((int64_t)1 << 32)) return -1;
        if (e.treeBytes != (e.numActive + 3) / 4) return -1;
        const int64_t rec = archive_record_bytes(g.D, g.maxDepth, e.treeBytes);
        if (e.offset > bytes || rec > bytes - e.offset) return -1;
    }
    std::atomic<int> bad(0);
    parallel_for(h.numBricks, [&](int b) {
        const ArchiveEntry &e = dir[(size_t)b];
        if (e.offset == 0) return;
        const int64_t rec = archive_record_bytes(g.D, g.maxDepth, e.treeBytes);
        if (fnv1a64((const uint8_t *)blob + e.offset, rec) != e.hash) { bad = 1; return; }
        if (!block_table_ok(g.D, e.numActive, archive_record(blob, g, e).blockOff)) bad = 1;
    });
    return bad ? -1 : 0;
}

bool archive_write(FILE *f, const ArchiveGeom &g, const std::vector<ArchiveBrick> &bricks)
{
    const int Dc = block_depth(g.D);
    const int64_t dirEnd = VR_ARCHIVE_HEADER_BYTES + (int64_t)g.numBricks * VR_ARCHIVE_ENTRY_BYTES;
    std::vector<ArchiveEntry> dir((size_t)g.numBricks, ArchiveEntry{0, 0, 0, 0});
    std::vector<std::vector<uint8_t>> recs((size_t)g.numBricks);
    parallel_for(g.numBricks, [&](int b) {
        const ArchiveBrick &k = bricks[(size_t)b];
        if (k.numActive <= 0) return;
        const int64_t tb = (k.numActive + 3) / 4;
        std::vector<uint8_t> &r = recs[(size_t)b];
        r.assign((size_t)archive_record_bytes(g.D, g.maxDepth, tb), 0);
        uint8_t *p = r.data();
        memcpy(p, k.dmap, (size_t)g.maxDepth + 1); p += pad16(g.maxDepth + 1);
        memcpy(p, k.topVal.data(), (size_t)2 << Dc); p += pad16((int64_t)2 << Dc);
        memcpy(p, k.blockOff.data(), (size_t)4 << Dc); p += pad16((int64_t)4 << Dc);
        memcpy(p, k.tree, (size_t)tb);
        dir[(size_t)b] = ArchiveEntry{0, tb, k.numActive, fnv1a64(r.data(), (int64_t)r.size())};
    });
    int64_t at = dirEnd;
    for (int b = 0; b < g.numBricks; ++b)
        if (!recs[(size_t)b].empty()) { dir[(size_t)b].offset = at; at += (int64_t)recs[(size_t)b].size(); }
    ArchiveHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, ARCHIVE_MAGIC, 8);
    h.version = 1; h.variant = (uint32_t)g.variant; h.numBricks = g.numBricks; h.D = g.D; h.maxDepth = g.maxDepth; h.fileBytes = at;
    for (int k = 0; k < 3; ++k) h.dims[k] = g.dims[k];
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1 && fwrite(dir.data(), VR_ARCHIVE_ENTRY_BYTES, dir.size(), f) == dir.size();
    for (int b = 0; ok && b < g.numBricks; ++b)
        if (!recs[(size_t)b].empty()) ok = fwrite(recs[(size_t)b].data(), 1, recs[(size_t)b].size(), f) == recs[(size_t)b].size();
    return ok;
}

bool read_header(FILE *f, Header &h)
{
    if (fread(&h, VR_HEADER_BYTES, 1, f) != 1) return false;
    return h.maxDepth >= VR_CHAIN_LEVELS && h.maxDepth < VR_MAX_DEPTH && h.numActive > 0;
}

bool write_header(FILE *f, const Header &h) { return fwrite(&h, VR_HEADER_BYTES, 1, f) == 1; }

// ---- the estimator's round plan (the census of threshold trajectories it was chosen from) ----
// On the bench volume half of the walks never change their threshold and a third of all changes fall into the first
// sixteenth of a level: a 4-wide prefix round over that sixteenth and a 2-wide one (oriented by the half of its interval
// the mean sits in) up to a quarter absorb them for a fraction of the level's segments, the bulk gets ONE candidate, a
// 4-wide quad round picks up the bricks that left it, and 8-wide exact rounds finish what is left.  A prefix shorter than
// EST_MIN_PREFIX segments is not worth its launches.
EstPlan est_round_plan(uint32_t nseg, bool oldSchedule)
{
    constexpr uint32_t first = VR_EST_HEAD / VR_EST_SEG, EST_MIN_PREFIX = 8;
    EstPlan p{};
    const auto add = [&](uint32_t end, int nc, bool quads, int sweeps = 4) { p.r[p.rounds++] = EstRound{end, nc, quads, sweeps}; };
    if (nseg <= first) return p;
    if (oldSchedule) {
        add(nseg, 4, true);
        add(nseg, 4, false);
    } else {
        const uint32_t len = nseg - first;
        uint32_t at = first;
        for (const int shift : {4, 2}) {
            const uint32_t pre = len >> shift;
            if (pre >= EST_MIN_PREFIX && first + pre > at) { at = first + pre; add(at, shift == 4 ? 4 : 2, true); }
        }
        add(nseg, 1, true);
        add(nseg, 4, true, 16);     // (4 and 8 sweeps measured: DESIGN.md 3.2)
    }
    for (int i = 0; i < 3; ++i) add(nseg, VR_EST_CAND, false);
    return p;
}

static uint32_t cdiv(int64_t a, int64_t b) { return (uint32_t)((a + b - 1) / b); }

EstLaunch est_launch(const EstRound &R, bool exactBounds, int32_t budget)
{
    const int64_t len = (int64_t)R.segEnd - VR_EST_HEAD / VR_EST_SEG;
    EstLaunch l{};
    l.gx = R.quads ? cdiv(len, 8 * R.sweeps) : std::min(cdiv(len, 8), 64u);
    l.quads = R.quads && !exactBounds;
    l.budget = l.quads ? budget : -1;
    return l;
}

// ---- the debugging switches ----
const SwitchRow VR_SWITCHES[] = {
    {"decode_walk", &Switches::decodeWalk},
    {"decode_fine_v1", &Switches::decodeFineV1},
    {"decode_quad", &Switches::decodeQuad},
    {"no_skip_blocks", &Switches::noSkipBlocks},
    {"no_uniform_blocks", &Switches::noUniformBlocks},
    {"no_uniform_decode", &Switches::noUniformDecode},
    {"pyramid_boxes", &Switches::pyramidBoxes},
    {"index_per_block", &Switches::indexPerBlock},
    {"est_exact_bounds", &Switches::estExactBounds},
    {"est_old_schedule", &Switches::estOldSchedule},
};
const int VR_NUM_SWITCHES = (int)(sizeof(VR_SWITCHES) / sizeof(VR_SWITCHES[0]));

bool Switches::*find_switch(const char *name)
{
    for (int i = 0; name && i < VR_NUM_SWITCHES; ++i)
        if (!strcmp(name, VR_SWITCHES[i].name)) return VR_SWITCHES[i].member;
    return nullptr;
}

void switch_env_name(const char *name, char *out, size_t cap)
{
    snprintf(out, cap, "VRHIP_%s", name);
    for (char *c = out; *c; ++c) if (*c >= 'a' && *c <= 'z') *c = (char)(*c - 'a' + 'A');
}

Switches switches_from_env()
{
    Switches w;
    char env[64];
    for (int i = 0; i < VR_NUM_SWITCHES; ++i) {
        switch_env_name(VR_SWITCHES[i].name, env, sizeof(env));
        w.*VR_SWITCHES[i].member = getenv(env) != nullptr;
    }
    if (const char *eb = getenv("VRHIP_EST_BUDGET")) { const int v = atoi(eb); if (v >= 0) w.estBudget = v; }
    return w;
}

// ---- the build ----
int build_side_streams(int variant, int B, int levelLoopStreams)
{
    if (variant == VR_VARIANT_MIDRANGE) return 1;
    const int p = std::min(levelLoopStreams, VR_MAX_PARTS);
    return (B < 16 * p || p < 2) ? 0 : p - 1;
}

BuildPlan make_build_plan(const BuildInputs &in)
{
    BuildPlan p{};
    const int D = in.D, B = in.B;
    const int64_t leaves = (int64_t)1 << D;
    p.D = D; p.B = B; p.maxEpochs = in.maxEpochs;
    p.midRange = in.variant == VR_VARIANT_MIDRANGE;
    p.guarded = in.variant != VR_VARIANT_RECOVER;
    p.fused = build_fused(D);
    p.leafless = p.fused && in.maxEpochs >= 1;
    // SkipBlocks needs k_pyramid12's constant bit in front and k_prune_emit12 behind, a prune that makes such blocks
    // one token (tolerance >= 1) and a level loop that runs
    p.skipBlocks = p.fused && in.use12 && in.tolerance >= 1 && in.maxEpochs >= 1 && D >= 14 && !in.sw.noSkipBlocks;
    // (both streams of a MidRangeTree too; needs the leaf prune and an epoch to exist)
    p.constClosedForm = in.maxEpochs >= 1 && in.tolerance >= 1 && D >= 1;
    p.zeroFill = in.maxEpochs <= 0;
    p.boxes = (int64_t)1 << block_depth(D);
    // pyramid: bottom 12 levels by k_pyramid12 when x-runs of 16 voxels exist (eight boxes per workgroup where they
    // share their 128-byte lines), the rest (and small / thin bricks) in rounds of <= 10 levels
    p.pyr12 = in.use12;
    p.pyr12Lines = in.use12 && in.lines && !in.sw.pyramidBoxes;
    p.pyr12Grid = !p.pyr12 ? 0u : (uint32_t)((int64_t)1 << (p.pyr12Lines ? D - 15 : D - 12));
    p.pyrSrcIdx = !p.pyr12 && in.generalGeom;
    for (int dLeaf = p.pyr12 ? D - 12 : D; dLeaf > 0 || (!p.pyr12 && p.pyrRounds == 0); ) {
        const int L = std::min(dLeaf, 10);
        p.pyr[p.pyrRounds++] = PyrRound{dLeaf, L, (uint32_t)((int64_t)1 << (dLeaf - L))};
        dLeaf -= L;
    }
    p.rootStride = (int64_t)1 << std::max(D - 10, 0);
    // level loop: a MidRangeTree's two streams do not depend on each other, nor do the bricks of a VolumeKdtree
    const int want = std::min(in.levelLoopStreams, VR_MAX_PARTS);
    p.parts = (p.midRange || B < 16 * want || want < 2) ? 1 : std::min(want, 1 + in.sideStreams);
    for (int i = 0; i <= p.parts; ++i) p.range[i] = (int32_t)((int64_t)B * i / p.parts);
    p.forkRange = p.midRange && in.sideStreams >= 1;
    p.estOldSchedule = in.sw.estOldSchedule; p.estExactBounds = in.sw.estExactBounds; p.estBudget = in.sw.estBudget;
    // prune: constant blocks of a leafless SkipBlocks build have a closed form (k_prune_emit12_const)
    p.uniformBlocks = p.skipBlocks && p.leafless && !p.midRange && !in.sw.noUniformBlocks;
    p.uniformGrid = cdiv(p.boxes, VR_PEC_BOXES);
    p.pruneGrid = p.fused ? (uint32_t)p.boxes : cdiv(leaves, 256);
    p.pruneFrom = p.fused ? D - 13 : D - 1;
    // convert
    p.emitLeaves = p.fused ? 4096 : VR_EMIT_RANKS;
    p.nblk = cdiv(leaves, p.emitLeaves);
    p.index = !p.fused ? VR_EMIT_WRITE : (in.sw.indexPerBlock ? VR_INDEX12_BLOCK : VR_INDEX12);
    p.indexGrid = p.index == VR_INDEX12 ? cdiv(p.nblk, VR_IDX_BLOCKS) : (p.index == VR_INDEX12_BLOCK ? cdiv(p.nblk, 4) : (uint32_t)p.nblk);
    // (k_index12 writes the index entries of constant bricks too; the other two leave them to k_const_finish)
    p.constFinishIdx = p.index == VR_INDEX12 ? 0 : (int64_t)1 << (D - std::min(D, 6));
    p.constFinishGrid = p.index == VR_INDEX12 ? 1u : cdiv(p.constFinishIdx, 256);
    p.constFinishThreads = p.index == VR_INDEX12 ? 64u : 256u;
    // statistics records: one per 1024 leaves from k_prune_emit12, one per 256 from k_prune_leaf
    p.statRecords = cdiv(leaves, p.fused ? 1024 : 256);
    p.gapped = p.fused;
    p.compact = p.fused && in.compactOnBuild;
    return p;
}

BuildLevel build_level(const BuildPlan &p, int d)
{
    BuildLevel l{};
    const int64_t n = (int64_t)1 << d;
    l.constLeaves = p.skipBlocks && d == p.D - 1;
    if (n > VR_EST_HEAD) {
        l.est = est_round_plan((uint32_t)(n / VR_EST_SEG), p.estOldSchedule);
        for (int r = 0; r < l.est.rounds; ++r) l.estL[r] = est_launch(l.est.r[r], p.estExactBounds, p.estBudget);
    }
    l.fill16 = n >= 4096;
    l.sumsOnly = p.leafless && d == p.D;
    l.iters = !l.fill16 ? 0 : (n / 4096 >= 512 ? FILL_ITERS : (n / 4096 >= 64 ? std::min(FILL_ITERS, 4) : 1));
    l.fillGrid = l.fill16 ? cdiv(n / 4096, l.iters) : cdiv(n, FILL_NODES_PER_BLOCK);
    return l;
}

// ---- a decode ----
static_assert(VR_STAGE_BRICKS == VR_POOL_STAGE_BRICKS, "the staged batches are the header's");

// the only place a decode kernel is chosen
static DecodeKernel decode_kernel(const DecodeInputs &in, int cut)
{
    if (in.generalGeom) return DecodeKernel::GENERAL;
    if (!in.tileOk) return DecodeKernel::LANE;
    const bool fine = in.fineAll && !in.rangeStream && !in.decodeWalk;
    // k_decode_region / k_decode_quad: cuts at or below depth D-3 (the third side-car holds the depth-(D-3) scalars
    // at full precision); shallower progressive cuts keep k_decode_fine, which decodes the upper nodes itself
    if (fine && in.idxVal3 && cut >= in.D - 3 && !in.decodeFineV1)
        return !in.decodeQuad && in.regionOk ? DecodeKernel::REGION : DecodeKernel::QUAD;
    return fine ? DecodeKernel::FINE : DecodeKernel::TILE;
}

// the tiled kernels store 16-byte vectors to their destination, k_decode_lane and k_owner_gather bytes
static bool stores_vectors(DecodeKernel k) { return k != DecodeKernel::GENERAL && k != DecodeKernel::LANE; }

static DecodeLaunch decode_class(const DecodeInputs &in, DecodeKernel k, int rows, int cut, bool perBrick)
{
    DecodeLaunch l{};
    l.kernel = k; l.rows = rows; l.cut = cut;
    switch (k) {
    case DecodeKernel::GENERAL:     // rank-domain decode, then every voxel takes its owner leaf's value
        l.gatherGx = cdiv(in.voxels, 256);
        [[fallthrough]];
    case DecodeKernel::LANE:
        l.gx = cdiv(in.nIdx, 64); l.threads = 64;
        break;
    case DecodeKernel::REGION:
        // a workgroup decodes every VR_RG_PER-th region of its brick: enough regions to amortise its tables and the
        // pipeline's fill, enough workgroups (a few thousand for the bench volume) to balance the chip
        l.gx = cdiv(in.nreg, VR_RG_PER); l.threads = 64 * VR_RG_WAVES;
        if ((int64_t)l.gx * rows < VR_RG_MIN_WGS) l.gx = (uint32_t)std::min<int64_t>(in.nreg, cdiv(VR_RG_MIN_WGS, rows));
        break;
    case DecodeKernel::QUAD:
        l.gx = cdiv(in.tiles, VR_QD_WAVES * VR_QD_TPW); l.threads = 64 * VR_QD_WAVES;
        l.chainLevels = perBrick ? 0 : std::min(std::max(cut - in.D, 0), VR_CHAIN_LEVELS);
        break;
    case DecodeKernel::FINE:
        l.gx = cdiv(in.tiles, VR_FD_WAVES); l.threads = 64 * VR_FD_WAVES; l.fineTables = true;
        break;
    case DecodeKernel::TILE:
        l.gx = cdiv(in.tiles, VR_DEC_WAVES); l.threads = 64 * VR_DEC_WAVES;
        break;
    }
    return l;
}

static void class_needs(DecodeNeeds &n, DecodeKernel k)
{
    n.rankVals = n.rankVals || k == DecodeKernel::GENERAL;
    n.decTables = n.decTables || k == DecodeKernel::FINE;       // (k_decode_quad's tables are chainTab; region and tile have none)
    n.chainTab = n.chainTab || k == DecodeKernel::QUAD;
}

DecodePlan make_decode_plan(const DecodeInputs &in, int cut)
{
    DecodePlan p{};
    const DecodeKernel k = decode_kernel(in, cut);
    p.launch = decode_class(in, k, in.B, cut, false);
    p.rangeStream = in.rangeStream;
    // MidRangeTree's second stream has no index scalars of its own: they are its cut values at depth Ds
    p.cutValues = cut < in.Ds || in.rangeStream ? (in.foreign ? CutSource::CALLER : CutSource::CODES) : CutSource::NONE;
    p.cutAll = std::min(cut, in.Ds);
    p.idxValFromCut = in.rangeStream;
    // the uniform hint describes the mid stream of this handle's own last build (an installed stream has none)
    p.uni = !in.foreign && !in.rangeStream && !in.noUniformDecode;
    p.nBase = k == DecodeKernel::GENERAL && in.idx64 ? in.nEmitBlk : 0;
    p.storesVectors = stores_vectors(k);
    class_needs(p.needs, k);
    p.needs.idxValCut = p.cutValues != CutSource::NONE;
    return p;
}

LodPlan make_lod_plan(const DecodeInputs &in, const int32_t *cuts, const uint8_t *topIndexed, const int64_t *off,
                      const uint8_t *shift, int64_t tableCells)
{
    LodPlan p{};
    const int B = in.B;
    const bool pool = off != nullptr;
    p.image.reserve((size_t)3 * B);
    p.image.assign(cuts, cuts + B);
    std::vector<DecodeKernel> kern((size_t)B);      // each decoded brick's kernel, chosen once
    for (int b = 0; b < B; ++b) if (cuts[b] >= 0) kern[(size_t)b] = decode_kernel(in, cuts[b]);
    for (int top = 1; top >= 0; --top) {
        for (int b = 0; b < B; ++b)
            if (cuts[b] >= 0 && cuts[b] < in.Ds && (in.foreign && topIndexed && topIndexed[b]) == (top == 1)) p.image.push_back(b);
        if (top) p.nTop = (int)p.image.size() - B;
    }
    p.nAbove = (int)p.image.size() - B;
    // the passes: [0] full resolution (every decoded brick without a pool), then the staged batches
    const auto coarse = [&](int b) { return pool && (shift[3 * b] | shift[3 * b + 1] | shift[3 * b + 2]) != 0; };
    std::vector<std::vector<int>> passes(1);
    passes[0].reserve((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (cuts[b] < 0) continue;
        if (!coarse(b)) { passes[0].push_back(b); p.storesVectors = p.storesVectors || stores_vectors(kern[(size_t)b]); continue; }
        if (passes.size() == 1 || (int)passes.back().size() == VR_STAGE_BRICKS) passes.emplace_back();
        passes.back().push_back(b);
        // k_pool_pack writes 32-bit words for stored rows of 4 bytes or more
        p.storesVectors = p.storesVectors || in.nb0 - shift[3 * b] >= 2;
    }
    p.staged = passes.size() > 1;
    if (pool) p.offsets.assign((size_t)B, 0);
    for (int ps = 0; ps < (int)passes.size(); ++ps) {
        const std::vector<int> &bricks = passes[(size_t)ps];
        for (int c = 0; c < DECODE_KERNELS; ++c) {
            const int first = (int)p.image.size();
            int cut = 0;
            for (int i = 0; i < (int)bricks.size(); ++i) {
                const int b = bricks[(size_t)i];
                if ((int)kern[(size_t)b] != c) continue;
                if (pool) p.offsets[p.image.size() - (size_t)(B + p.nAbove)] = ps == 0 ? off[b] : (int64_t)i * in.voxels;
                p.image.push_back(b);
                cut = cuts[b];
            }
            const int n = (int)p.image.size() - first;
            if (!n) continue;
            DecodeLaunch l = decode_class(in, (DecodeKernel)c, n, cut, true);
            l.pass = ps; l.first = first;
            l.waitStage = ps == 1 && (p.launches.empty() || p.launches.back().pass == 0);
            p.launches.push_back(l);
            class_needs(p.needs, l.kernel);
        }
        if (ps == 0) continue;
        p.launches.back().packRows = (int)bricks.size();
        p.launches.back().packFirst = ((int)p.offsets.size() - B) / 2;
        for (int b : bricks) {
            p.offsets.push_back(off[b]);
            p.offsets.push_back(shift[3 * b] | (shift[3 * b + 1] << 8) | (shift[3 * b + 2] << 16));
        }
    }
    p.nRows = (int)p.image.size() - B - p.nAbove;
    p.packGx = (uint32_t)std::min<int64_t>(1024, (in.voxels / 4 + 255) / 256);
    p.cutValues = !p.nAbove ? CutSource::NONE : (in.foreign ? CutSource::CALLER : CutSource::CODES);
    p.uni = !in.foreign && !in.noUniformDecode;
    p.nBase = in.generalGeom && in.idx64 ? in.nEmitBlk : 0;
    p.needs.idxValCut = p.nAbove != 0;
    p.tableCells = tableCells;
    p.nothing = p.nRows == 0 && p.nAbove == 0 && tableCells == 0;
    return p;
}

int pool_layout(const int64_t bd[3], int32_t nb, const int64_t *ijk, const int64_t grid[3], const int32_t *cuts,
                int32_t origDepth, int32_t maxDepth, int64_t *off, uint8_t *shift, vr_pool_entry *table, int64_t *total)
{
    if (!bd || !ijk || !grid || !cuts || !total || nb <= 0) return VR_ERR_INVALID;
    int lg[3];
    for (int k = 0; k < 3; ++k) {
        if (bd[k] <= 0 || (bd[k] & (bd[k] - 1)) != 0 || bd[k] >= (1ll << 31) || grid[k] <= 0) return VR_ERR_INVALID;
        lg[k] = 0;
        while (((int64_t)1 << lg[k]) < bd[k]) ++lg[k];
    }
    if (origDepth != lg[0] + lg[1] + lg[2] || maxDepth < origDepth) return VR_ERR_INVALID;
    const int64_t cells = grid[0] * grid[1] * grid[2];
    std::vector<int64_t> cellOf((size_t)nb);
    const std::vector<std::array<int, 3>> splits = split_counts(bd, origDepth);
    int64_t run = 0;
    for (int32_t b = 0; b < nb; ++b) {
        const int64_t *q = ijk + 3 * (int64_t)b;
        for (int k = 0; k < 3; ++k) if (q[k] < 0 || q[k] >= grid[k]) return VR_ERR_INVALID;
        const int c = cuts[b];
        if (c < -1 || c > maxDepth) return VR_ERR_INVALID;
        cellOf[(size_t)b] = q[0] + grid[0] * (q[1] + grid[1] * q[2]);
        uint8_t sh[3] = {0, 0, 0};
        if (c >= 0 && c < origDepth)
            for (int k = 0; k < 3; ++k) sh[k] = (uint8_t)(lg[k] - splits[(size_t)c][(size_t)k]);
        if (shift) for (int k = 0; k < 3; ++k) shift[3 * b + k] = sh[k];
        int64_t o = -1;
        if (c >= 0) {
            o = (run + 255) & ~(int64_t)255;
            run = o + ((bd[0] >> sh[0]) * (bd[1] >> sh[1]) * (bd[2] >> sh[2]));
        }
        if (off) off[b] = o;
    }
    std::vector<int64_t> cs = cellOf;       // two bricks on one cell: refused
    std::sort(cs.begin(), cs.end());
    if (std::adjacent_find(cs.begin(), cs.end()) != cs.end()) return VR_ERR_INVALID;
    for (int64_t cell = 0; table && cell < cells; ++cell) { table[cell] = vr_pool_entry(); table[cell].offset = -1; }
    for (int32_t b = 0; table && b < nb; ++b) {
        if (cuts[b] < 0) continue;
        vr_pool_entry &e = table[cellOf[(size_t)b]];
        e.offset = off[b];
        for (int k = 0; k < 3; ++k) e.shift[k] = shift[3 * b + k];
    }
    *total = run;
    return VR_OK;
}

} // namespace vr

// ---- error-bounded selection of cuts: the rule is stated in vrhip.h ("error-bounded level of detail") ----
extern "C" vr_status vr_lod_select_error(const vr_brick_error *table, int32_t num_bricks, int32_t cut_lo, int32_t cut_hi,
                                         int64_t voxels_per_brick, const int32_t *cuts_in, int32_t max_abs_bound,
                                         double mean_sq_bound, int32_t *cuts_out)
{
    if (!table || !cuts_out || num_bricks < 1 || cut_lo < 0 || cut_lo > cut_hi || voxels_per_brick < 1) return VR_ERR_INVALID;
    if (max_abs_bound < 0 || mean_sq_bound != mean_sq_bound) return VR_ERR_INVALID;
    for (int32_t b = 0; cuts_in && b < num_bricks; ++b) if (cuts_in[b] < -1) return VR_ERR_INVALID;
    for (int32_t b = 0; b < num_bricks; ++b) {
        const int32_t h = cuts_in ? cuts_in[b] : cut_hi;
        int32_t pick = h;
        for (int32_t c = cut_lo; h >= 0 && c <= std::min(h, cut_hi); ++c) {
            const vr_brick_error &e = table[(int64_t)(c - cut_lo) * num_bricks + b];
            if (e.max_abs > (uint32_t)max_abs_bound) continue;
            if (mean_sq_bound >= 0.0 && !((double)e.sum_sq <= mean_sq_bound * (double)voxels_per_brick)) continue;
            pick = c;
            break;
        }
        cuts_out[b] = pick;
    }
    return VR_OK;
}

// ---- the block table of a stream: the definition is in host_plan.h, the contract in vrhip.h ----
extern "C" vr_status vr_stream_block_table(const int64_t dims[3], const uint8_t *tree_host, int64_t tree_bytes, int64_t num_active,
                                           const uint8_t *dmap, int32_t map_len, uint32_t *block_off_out, uint8_t *top_val_out)
{
    if (!dims || !tree_host || !dmap || !block_off_out || !top_val_out || num_active <= 0) return VR_ERR_INVALID;
    for (int k = 0; k < 3; ++k) if (dims[k] <= 0 || dims[k] > (1ll << 20)) return VR_ERR_INVALID;
    if (dims[0] * dims[1] * dims[2] >= (1ll << 32)) return VR_ERR_UNSUPPORTED;
    vr::Geom g;
    vr::make_geom(g, dims);
    if (g.D > 31 || num_active >= (1ll << 32)) return VR_ERR_UNSUPPORTED;
    if (map_len < g.D + VR_CHAIN_LEVELS + 1) return VR_ERR_INVALID;
    if (tree_bytes < (num_active + 3) / 4) return VR_ERR_FORMAT;
    return vr::block_table_from_stream(g.D, tree_host, num_active, dmap, block_off_out, top_val_out) == 0 ? VR_OK : VR_ERR_FORMAT;
}

// ---- a display window from a histogram's percentiles: the rule is stated in vrhip.h ("volume histograms") ----
extern "C" vr_status vr_window_from_histogram(const uint64_t *hist, int32_t first_bin, double lo_fraction, double hi_fraction,
                                              float *window_lo, float *window_hi)
{
    if (!hist || !window_lo || !window_hi || first_bin < 0 || first_bin > 255) return VR_ERR_INVALID;
    if (!(lo_fraction >= 0.0 && lo_fraction <= 1.0) || !(hi_fraction >= 0.0 && hi_fraction <= 1.0)) return VR_ERR_INVALID;   // (NaN too)
    if (lo_fraction > hi_fraction) return VR_ERR_INVALID;
    uint64_t n = 0;
    for (int k = first_bin; k < 256; ++k) n += hist[k];
    if (n == 0) return VR_ERR_INVALID;
    const double lo_at = lo_fraction * (double)n, hi_at = hi_fraction * (double)n;
    int lo_k = -1, hi_k = -1, last = first_bin;
    uint64_t cum = 0;
    for (int k = first_bin; k < 256; ++k) {
        cum += hist[k];
        if (hist[k] != 0) last = k;
        if (lo_k < 0 && (double)cum > lo_at) lo_k = k;
        if (hi_k < 0 && (double)cum >= hi_at) hi_k = k;
    }
    if (lo_k < 0) lo_k = last;
    if (hi_k < 0) hi_k = 255;                  // (cum_255 = N >= hi_fraction N: never taken)
    if (hi_k <= lo_k) hi_k = lo_k + 1;
    if (hi_k > 255) { --lo_k; --hi_k; }
    *window_lo = (float)lo_k / 255.0f;
    *window_hi = (float)hi_k / 255.0f;
    return VR_OK;
}
