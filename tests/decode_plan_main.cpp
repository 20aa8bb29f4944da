// decode_plan_main.cpp -- the plan of a decode call (volumerenderer_amd/csrc/host_plan.cpp: make_decode_plan,
// make_lod_plan, pool_layout), stand-alone: tests/test_decode_plan.py builds it under the address and
// undefined-behaviour sanitizers.  No device, no Python.
//   usage: decode_plan_main
// Restates the rules of vr_brickset_decode / _decode_range / _decode_lod / _decode_lod_pool in its own words -- it calls
// nothing of the unit but the functions under test -- and compares every field of the plans.
// Uniform decodes, the cross product of
//   D 0 .. 30 (K = min(D, 6), Ds = D - K); cuts 0, Ds-1, Ds, D-4, D-3, D, D+1, D+7 (= maxDepth), those inside [0, D+7];
//   tile.ok, region.ok, generalGeom, idx64, the fine side-car, idxVal3, foreign, rangeStream on and off;
//   none, each and all of decode_walk, decode_fine_v1, decode_quad, no_uniform_decode;
//   (B, tiles, nreg) so that rows x workgroups of k_decode_region lies on both sides of 2048 and at it.
// Per-brick decodes: B 1 2 33 65 VR_MAX_BRICKS; the cut patterns all skipped / all full / all above Ds / every class the
// inputs allow; without a pool and with 0, 1, 32, 33, 65 coarse bricks (first ones or every other one; narrow or wide
// stored rows); own streams, and foreign ones with no, every third or all bricks top-indexed; five kernel settings
// (at VR_MAX_BRICKS: the tiled and the general setting, own streams and every third brick top-indexed).
// Asserted per plan: every decoded brick is in exactly one class list, lists and offsets stay within 3B entries, the
// classes tile the lists in pass and kernel order, descriptors follow batch order, and storesVectors / needs equal the
// restated rules.  pool_layout: 256-byte slots, two bricks on one cell refused, shifts and total against a restated sum.
// Prints "decode plans: <n> ok", "lod plans: <n> ok", "pool layouts: <n> ok".
#include "../volumerenderer_amd/csrc/host_plan.h"
#include "../include/vrhip.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>

using namespace vr;

static char g_case[320];
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_case); exit(1); } } while (0)

static int64_t up(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- the rules, restated ----
static DecodeKernel want_kernel(const DecodeInputs &in, int cut)
{
    if (in.generalGeom) return DecodeKernel::GENERAL;           // tables at both ends, whatever else the set has
    if (!in.tileOk) return DecodeKernel::LANE;
    if (in.rangeStream || in.decodeWalk || !in.fineAll) return DecodeKernel::TILE;      // no per-4-leaf counts to use
    if (in.decodeFineV1 || !in.idxVal3 || cut < in.D - 3) return DecodeKernel::FINE;
    if (in.decodeQuad || !in.regionOk) return DecodeKernel::QUAD;
    return DecodeKernel::REGION;
}
static bool tiled(DecodeKernel k) { return k == DecodeKernel::REGION || k == DecodeKernel::QUAD || k == DecodeKernel::FINE || k == DecodeKernel::TILE; }

static void check_class(const DecodeInputs &in, const DecodeLaunch &l, DecodeKernel k, int rows, int cut, bool perBrick)
{
    REQUIRE(l.kernel == k && l.rows == rows && l.cut == cut && rows >= 1);
    REQUIRE(l.fineTables == (k == DecodeKernel::FINE));
    REQUIRE((l.gatherGx != 0) == (k == DecodeKernel::GENERAL));
    int levels = 0;
    switch (k) {
    case DecodeKernel::GENERAL:
        REQUIRE((int64_t)l.gatherGx == up(in.voxels, 256));
        /* fall through */
    case DecodeKernel::LANE:
        REQUIRE(l.threads == 64 && (int64_t)l.gx == up(in.nIdx, 64));
        break;
    case DecodeKernel::REGION: {
        int64_t g = up(in.nreg, 16);
        if (g * rows < 2048) g = std::min<int64_t>(in.nreg, up(2048, rows));
        REQUIRE(l.threads == 512 && (int64_t)l.gx == g);
        REQUIRE((int64_t)l.gx * VR_RG_PER >= in.nreg && (int64_t)l.gx <= in.nreg && l.gx >= 1);      // every region has a workgroup, no workgroup is idle
        break;
    }
    case DecodeKernel::QUAD:
        REQUIRE(l.threads == 1024 && (int64_t)l.gx == up(in.tiles, 256));
        levels = perBrick ? 0 : (cut <= in.D ? 0 : (cut - in.D >= 7 ? 7 : cut - in.D));
        break;
    case DecodeKernel::FINE:
    case DecodeKernel::TILE:
        REQUIRE(l.threads == 256 && (int64_t)l.gx == up(in.tiles, 4));
        break;
    }
    REQUIRE(l.chainLevels == levels);
}

static long check_decode(const DecodeInputs &in, int cut)
{
    snprintf(g_case, sizeof(g_case), "D %d Ds %d B %d cut %d tiles %d nreg %d tile %d region %d general %d idx64 %d fine %d val3 %d foreign %d range %d sw %d%d%d%d",
             in.D, in.Ds, in.B, cut, in.tiles, in.nreg, in.tileOk, in.regionOk, in.generalGeom, in.idx64, in.fineAll, in.idxVal3, in.foreign,
             in.rangeStream, in.decodeWalk, in.decodeFineV1, in.decodeQuad, in.noUniformDecode);
    const DecodePlan p = make_decode_plan(in, cut);
    const DecodeKernel k = want_kernel(in, cut);
    check_class(in, p.launch, k, in.B, cut, false);
    REQUIRE(p.launch.pass == 0 && p.launch.packRows == 0 && !p.launch.waitStage);
    const bool above = cut < in.Ds || in.rangeStream;
    REQUIRE(p.rangeStream == in.rangeStream && p.idxValFromCut == in.rangeStream);
    REQUIRE(p.cutValues == (!above ? CutSource::NONE : (in.foreign ? CutSource::CALLER : CutSource::CODES)));
    REQUIRE(p.cutAll == (cut < in.Ds ? cut : in.Ds));
    REQUIRE(p.uni == !(in.foreign || in.rangeStream || in.noUniformDecode));
    REQUIRE(p.nBase == (in.generalGeom && in.idx64 ? in.nEmitBlk : 0));
    REQUIRE(p.storesVectors == tiled(k));
    REQUIRE(p.needs.rankVals == (k == DecodeKernel::GENERAL) && p.needs.decTables == (k == DecodeKernel::FINE));
    REQUIRE(p.needs.chainTab == (k == DecodeKernel::QUAD) && p.needs.idxValCut == above);
    return 1;
}

static DecodeInputs inputs(int D, int B)
{
    DecodeInputs in{};
    in.D = D; in.Ds = D - std::min(D, 6); in.B = B; in.nb0 = (D + 2) / 3;
    in.nIdx = (int64_t)1 << in.Ds; in.voxels = (int64_t)1 << D; in.leafStride = in.voxels; in.nEmitBlk = up(in.voxels, 256);
    in.tiles = (int)std::max<int64_t>(1, in.voxels >> 9); in.nreg = (int)std::max<int64_t>(1, in.voxels >> 12);
    return in;
}

static long uniform_plans()
{
    long n = 0;
    // rows x ceil(nreg / 16) below, at and above 2048; nreg smaller than the workgroups asked for; one brick
    static const int shape[][3] = {{1, 1, 1}, {1, 5, 15}, {7, 255, 17}, {64, 256, 512}, {128, 257, 256}, {127, 4096, 256}, {129, 4096, 255},
                                   {2048, 8, 16}, {2049, 8, 1}, {4, 100000, 8192}, {65535, 64, 3}};
    for (int D = 0; D <= 30; ++D)
        for (const auto &s : shape) {
            DecodeInputs base = inputs(D, s[0]);
            base.tiles = s[1]; base.nreg = s[2];
            const int cuts[] = {0, base.Ds - 1, base.Ds, D - 4, D - 3, D, D + 1, D + VR_CHAIN_LEVELS};
            for (int flags = 0; flags < 256; ++flags)
                for (int sw = 0; sw < 6; ++sw) {
                    DecodeInputs in = base;
                    in.tileOk = flags & 1; in.regionOk = flags & 2; in.generalGeom = flags & 4; in.idx64 = flags & 8;
                    in.fineAll = flags & 16; in.idxVal3 = flags & 32; in.foreign = flags & 64; in.rangeStream = flags & 128;
                    in.decodeWalk = sw == 1 || sw == 5; in.decodeFineV1 = sw == 2 || sw == 5; in.decodeQuad = sw == 3 || sw == 5;
                    in.noUniformDecode = sw == 4 || sw == 5;
                    for (int cut : cuts) if (cut >= 0 && cut <= D + VR_CHAIN_LEVELS) n += check_decode(in, cut);
                }
        }
    return n;
}

// ---- per-brick decodes ----
static long check_lod(const DecodeInputs &in, const std::vector<int32_t> &cuts, const uint8_t *top, const int64_t *off, const uint8_t *shift,
                      int64_t cells)
{
    const int B = in.B;
    const LodPlan p = make_lod_plan(in, cuts.data(), top, off, shift, cells);
    const bool pool = off != nullptr;
    const auto isCoarse = [&](int b) { return pool && (shift[3 * b] || shift[3 * b + 1] || shift[3 * b + 2]); };
    // the image: the cuts, then the bricks cut above Ds, those served by idxTop first
    REQUIRE((int)p.image.size() >= B && std::equal(cuts.begin(), cuts.end(), p.image.begin()));
    std::vector<int32_t> above;
    for (int t = 0; t < 2; ++t)
        for (int b = 0; b < B; ++b) {
            const bool isTop = in.foreign && top && top[b];
            if (cuts[b] >= 0 && cuts[b] < in.Ds && isTop == (t == 0)) above.push_back(b);
            if (t == 0 && b == B - 1) REQUIRE(p.nTop == (int)above.size());
        }
    REQUIRE(p.nAbove == (int)above.size() && (int)p.image.size() >= B + p.nAbove);
    REQUIRE(std::equal(above.begin(), above.end(), p.image.begin() + B));
    // every decoded brick in exactly one list
    int decoded = 0, nCoarse = 0;
    std::vector<int> rank((size_t)B, -1);       // of a coarse brick among the coarse ones, in index order
    for (int b = 0; b < B; ++b) if (cuts[b] >= 0) { ++decoded; if (isCoarse(b)) rank[(size_t)b] = nCoarse++; }
    REQUIRE(p.nRows == decoded && (int)p.image.size() == B + p.nAbove + decoded && p.image.size() <= (size_t)3 * B);
    std::vector<uint8_t> seen((size_t)B, 0);
    for (int r = 0; r < decoded; ++r) {
        const int b = p.image[(size_t)(B + p.nAbove + r)];
        REQUIRE(b >= 0 && b < B && cuts[b] >= 0 && !seen[(size_t)b]);
        seen[(size_t)b] = 1;
    }
    REQUIRE(p.offsets.size() == (pool ? (size_t)B + 2 * (size_t)nCoarse : 0) && p.offsets.size() <= (size_t)3 * B);
    // the classes tile the lists: pass by pass, inside a pass in the kernels' order, bricks in index order
    int at = B + p.nAbove, prevPass = 0, prevKernel = -1;
    bool anyK[DECODE_KERNELS] = {}, vectors = false, waited = false;
    for (size_t li = 0; li < p.launches.size(); ++li) {
        const DecodeLaunch &l = p.launches[li];
        REQUIRE(l.first == at && l.pass >= prevPass);
        if (l.pass != prevPass) prevKernel = -1;
        REQUIRE((int)l.kernel > prevKernel);
        prevPass = l.pass; prevKernel = (int)l.kernel;
        check_class(in, l, l.kernel, l.rows, cuts[p.image[(size_t)(at + l.rows - 1)]], true);
        for (int r = 0; r < l.rows; ++r) {
            const int b = p.image[(size_t)(at + r)];
            REQUIRE(want_kernel(in, cuts[b]) == l.kernel);
            REQUIRE(r == 0 || b > p.image[(size_t)(at + r - 1)]);
            REQUIRE(l.pass == (isCoarse(b) ? 1 + rank[(size_t)b] / VR_POOL_STAGE_BRICKS : 0));
            if (pool) REQUIRE(p.offsets[(size_t)(at + r - B - p.nAbove)] == (isCoarse(b) ? (int64_t)(rank[(size_t)b] % VR_POOL_STAGE_BRICKS) * in.voxels : off[b]));
        }
        at += l.rows;
        anyK[(int)l.kernel] = true;
        const bool firstStaged = l.pass >= 1 && !waited;
        REQUIRE(l.waitStage == firstStaged);
        waited = waited || firstStaged;
        const bool lastOfBatch = l.pass >= 1 && (li + 1 == p.launches.size() || p.launches[li + 1].pass != l.pass);
        const int batch = lastOfBatch ? std::min(VR_POOL_STAGE_BRICKS, nCoarse - (l.pass - 1) * VR_POOL_STAGE_BRICKS) : 0;
        REQUIRE(l.packRows == batch && l.packFirst == (lastOfBatch ? (l.pass - 1) * VR_POOL_STAGE_BRICKS : 0));
    }
    REQUIRE(at == (int)p.image.size());
    REQUIRE(prevPass == (nCoarse + VR_POOL_STAGE_BRICKS - 1) / VR_POOL_STAGE_BRICKS);
    // descriptors: the coarse bricks in index order, which is batch order
    for (int b = 0; b < B; ++b) {
        if (cuts[b] < 0) continue;
        vectors = vectors || (isCoarse(b) ? in.nb0 - shift[3 * b] >= 2 : tiled(want_kernel(in, cuts[b])));
        if (rank[(size_t)b] < 0) continue;
        REQUIRE(p.offsets[(size_t)(B + 2 * rank[(size_t)b])] == off[b]);
        REQUIRE(p.offsets[(size_t)(B + 2 * rank[(size_t)b] + 1)] == (shift[3 * b] | shift[3 * b + 1] << 8 | shift[3 * b + 2] << 16));
    }
    REQUIRE(p.storesVectors == vectors);
    REQUIRE(p.staged == (nCoarse > 0) && (int64_t)p.packGx == std::min<int64_t>(1024, up(in.voxels / 4, 256)));
    REQUIRE(p.cutValues == (above.empty() ? CutSource::NONE : (in.foreign ? CutSource::CALLER : CutSource::CODES)));
    REQUIRE(p.uni == !(in.foreign || in.noUniformDecode) && p.nBase == (in.generalGeom && in.idx64 ? in.nEmitBlk : 0));
    REQUIRE(p.needs.idxValCut == !above.empty() && p.needs.rankVals == anyK[(int)DecodeKernel::GENERAL]);
    REQUIRE(p.needs.decTables == anyK[(int)DecodeKernel::FINE] && p.needs.chainTab == anyK[(int)DecodeKernel::QUAD]);
    REQUIRE(p.tableCells == cells && p.nothing == (decoded == 0 && cells == 0));
    return 1;
}

static long lod_plans()
{
    long n = 0;
    const int D = 18;       // 64^3: Ds 12; cuts 3 (above Ds), 12, 14 (fine), 15, 18, 25 (region / quad)
    const int Bs[] = {1, 2, 33, 65, VR_MAX_BRICKS};
    for (int B : Bs)
        for (int setting = 0; setting < 5; ++setting)
            for (int foreign = 0; foreign < 4; ++foreign)      // own streams; foreign with no / every third / every brick top-indexed
                for (int pattern = 0; pattern < 5; ++pattern)
                    for (int coarse = -1; coarse <= 65; coarse = coarse < 0 ? 0 : (coarse == 0 ? 1 : (coarse == 1 ? 32 : coarse + (coarse == 32 ? 1 : 32))))
                        for (int form = 0; form < (coarse > 0 ? 4 : 1); ++form) {
                            if (B == VR_MAX_BRICKS && (setting % 3 != 0 || foreign % 2 != 0)) continue;     // (the largest set: two settings, two origins)
                            DecodeInputs in = inputs(D, B);
                            in.tileOk = setting != 4; in.regionOk = true; in.fineAll = setting != 2; in.idxVal3 = true;
                            in.decodeQuad = setting == 1; in.generalGeom = setting == 3; in.idx64 = setting == 3;
                            in.foreign = foreign != 0; in.noUniformDecode = pattern == 1;
                            snprintf(g_case, sizeof(g_case), "lod B %d setting %d foreign %d pattern %d coarse %d form %d", B, setting, foreign, pattern, coarse, form);
                            static const int mix[] = {-1, 3, 12, 14, 15, 18, 25, 0};
                            std::vector<int32_t> cuts((size_t)B);
                            std::vector<uint8_t> top((size_t)B), shift((size_t)3 * B, 0);
                            std::vector<int64_t> off((size_t)B, -1);
                            int left = coarse;
                            for (int b = 0; b < B; ++b) {
                                cuts[(size_t)b] = pattern == 0 ? -1 : (pattern == 1 ? D + 7 : (pattern == 2 ? 3 : (pattern == 3 ? mix[b % 8] : mix[(b * 5 + 1) % 8])));
                                top[(size_t)b] = foreign == 3 || (foreign == 2 && b % 3 == 0);
                                if (cuts[(size_t)b] < 0) continue;
                                off[(size_t)b] = (int64_t)b * 256 * 1024;
                                if (left > 0 && ((form & 1) == 0 || b % 2 == 1)) {    // the first decoded bricks, or every other one
                                    --left;
                                    shift[(size_t)3 * b] = (form & 2) ? (uint8_t)(in.nb0 - 1) : 1;     // stored rows of 2 bytes, or of 32
                                    shift[(size_t)3 * b + 1] = (uint8_t)(b % 3);
                                }
                            }
                            const bool pool = coarse >= 0;
                            n += check_lod(in, cuts, foreign >= 2 ? top.data() : nullptr, pool ? off.data() : nullptr, pool ? shift.data() : nullptr,
                                           pool && (form & 1) == 0 && pattern != 2 ? 80 : 0);
                        }
    return n;
}

// ---- pool_layout ----
static long pool_layouts()
{
    long n = 0;
    const int64_t dimsOf[][3] = {{64, 64, 64}, {16, 16, 16}, {128, 32, 8}, {1, 1, 1}};
    for (const auto &bd : dimsOf)
        for (int nb : {1, 2, 33, 65}) {
            int lg[3] = {0, 0, 0};
            for (int k = 0; k < 3; ++k) while (((int64_t)1 << lg[k]) < bd[k]) ++lg[k];
            const int D = lg[0] + lg[1] + lg[2], maxDepth = D + VR_CHAIN_LEVELS;
            const int64_t grid[3] = {5, 4, 4};
            snprintf(g_case, sizeof(g_case), "pool %lld x %lld x %lld nb %d", (long long)bd[0], (long long)bd[1], (long long)bd[2], nb);
            std::vector<int64_t> ijk((size_t)3 * nb), off((size_t)nb);
            std::vector<int32_t> cuts((size_t)nb);
            std::vector<uint8_t> sh((size_t)3 * nb);
            std::vector<vr_pool_entry> tab(80);
            for (int b = 0; b < nb; ++b) {
                const int cell = (b * 7) % 80;      // 7 and 80 are coprime: no cell twice
                ijk[(size_t)3 * b] = cell % 5; ijk[(size_t)3 * b + 1] = cell / 5 % 4; ijk[(size_t)3 * b + 2] = cell / 20;
                cuts[(size_t)b] = b % (maxDepth + 2) - 1;       // -1 .. maxDepth
            }
            int64_t total = -1;
            REQUIRE(pool_layout(bd, nb, ijk.data(), grid, cuts.data(), D, maxDepth, off.data(), sh.data(), tab.data(), &total) == VR_OK);
            int64_t run = 0;
            int present = 0;
            for (int b = 0; b < nb; ++b) {
                const int c = cuts[(size_t)b];
                const uint8_t *s = &sh[(size_t)3 * b];
                // a node of depth c < D is a box of 2^(D - c) voxels; at or below the leaves, and skipped: no shift
                REQUIRE(s[0] + s[1] + s[2] == (c >= 0 && c < D ? D - c : 0) && s[0] <= lg[0] && s[1] <= lg[1] && s[2] <= lg[2]);
                if (c < 0) { REQUIRE(off[(size_t)b] == -1); continue; }
                ++present;
                REQUIRE(off[(size_t)b] % 256 == 0 && off[(size_t)b] >= run && off[(size_t)b] < run + 256);
                run = off[(size_t)b] + ((bd[0] * bd[1] * bd[2]) >> (s[0] + s[1] + s[2]));
                const vr_pool_entry &e = tab[(size_t)((b * 7) % 80)];
                REQUIRE(e.offset == off[(size_t)b] && !memcmp(e.shift, s, 3));
            }
            REQUIRE(total == run);
            int live = 0;
            for (const vr_pool_entry &e : tab) { REQUIRE(e.offset >= -1); live += e.offset >= 0; }
            REQUIRE(live == present);
            ++n;
            if (nb < 2) continue;
            for (int k = 0; k < 3; ++k) ijk[(size_t)3 * (nb - 1) + k] = ijk[(size_t)k];      // two bricks on one cell
            REQUIRE(pool_layout(bd, nb, ijk.data(), grid, cuts.data(), D, maxDepth, off.data(), sh.data(), nullptr, &total) == VR_ERR_INVALID);
            ++n;
        }
    return n;
}

int main()
{
    printf("decode plans: %ld ok\n", uniform_plans());
    printf("lod plans: %ld ok\n", lod_plans());
    printf("pool layouts: %ld ok\n", pool_layouts());
    return 0;
}
