// install_plan_main.cpp -- the plan of an install (volumerenderer_amd/csrc/host_plan.cpp: check_stream,
// make_install_plan; host_plan.h: std_chain_distances, install_fine_has), stand-alone: tests/test_install_plan.py builds
// it under the address and undefined-behaviour sanitizers.  No device, no Python.
//   usage: install_plan_main
// Restates the rules of vr_brickset_set_tree / vr_brickset_set_trees in its own words -- it calls nothing of the unit
// but the functions under test -- and compares every field of the plans.
//
// The precedence of the refusals, as the entry points had it before there was a plan (capi.hip, one commit earlier):
//   vr_brickset_set_tree   1 INVALID      null handle, stream or map; brick outside [0, B)
//                          2 INVALID      map_len < maxDepth + 1; num_active <= 0
//                          3 UNSUPPORTED  num_active >= 2^32
//                          4 STATE        a built set that is not one of installed streams
//                          5 FORMAT       tree_bytes < need or need > treeCap, need = (num_active + 3) / 4
//                            (no variant and no offset width is refused; then FORMAT from the host parse, which is not the plan's)
//   vr_brickset_set_trees  1 INVALID      null handle, brick list or descriptors; count outside [1, B]
//                          2 UNSUPPORTED  a MidRangeTree set, or 64-bit token offsets
//                          3 STATE        as above -- here in front of everything a stream can say
//                          4 stream by stream, in the order of the call, for each the first of:
//                              INVALID      brick outside [0, B) or named by an earlier entry
//                              INVALID      null stream or map; one table pointer null and the other not
//                              INVALID      map_len < maxDepth + 1; num_active <= 0
//                              UNSUPPORTED  num_active >= 2^32
//                              FORMAT       as above
// so a stream's INVALID and UNSUPPORTED beat STATE in set_tree and lose to it in set_trees, and an earlier stream's
// FORMAT beats a later stream's INVALID.
//
// The cross product of
//   D 3 5 6 11 12 13 20 (across D < 6, D < 12 and Dc > 0); K = 6 and K = min(D, 4); both engines; idx64 on and off; the
//   three variants; the four states of (built, foreign); stream slots of 3000 bytes and of 2^31;
//   calls of 1, 2 and B = 3 bricks, tables given and not;
//   a violation in each entry of the call, and (calls of two) in both entries at once, every ordered pair: a null stream, a null map,
//   either table pointer null alone, map_len = maxDepth, num_active 0, 2^32 - 1 (fits the large slots only) and 2^32,
//   tree_bytes = need - 1, need = treeCap + 1, need = treeCap (no refusal: tail 0), a brick named twice, brick = B,
//   brick = -1; and a null brick list, null descriptors, count 0 and count B + 1;
//   maps with each of the seven grown-branch distances one above and one below the standard one.
// Prints "install plans: <n> ok", "stream checks: <n> ok".
#include "../volumerenderer_amd/csrc/host_plan.h"
#include "../include/vrhip.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>

using namespace vr;

static char g_case[320];
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_case); exit(1); } } while (0)

static const int B = 3;
static const uint8_t STD_CHAIN[VR_CHAIN_LEVELS] = {64, 32, 16, 8, 4, 2, 1};
static const uint8_t g_bytes[16] = {0};         // never read: the plan looks at no stream and no table
static const uint32_t g_table[1] = {0};

enum Violation { NONE, NULL_TREE, NULL_MAP, NULL_OFF, NULL_TOP, SHORT_MAP, NA_ZERO, NA_MAX, NA_2P32, SHORT_BYTES, OVER_CAP, AT_CAP,
                 TWICE, BRICK_B, BRICK_NEG, NUM_VIOLATIONS };

// ---- the rules, restated ----
static int64_t bytes_of(int64_t tokens) { return tokens / 4 + (tokens % 4 != 0); }

// what one stream says on its own: the refusal classes it falls into
struct Says { bool invalid, unsupported, format; int64_t need; };
static Says stream_says(const vr_tree_desc &d, int maxDepth, int64_t cap)
{
    Says s{};
    s.invalid = !d.tree || !d.distance_map || (!d.block_off != !d.top_val) || d.map_len <= maxDepth || d.num_active < 1;
    s.unsupported = d.num_active > 0xFFFFFFFFll;
    s.need = bytes_of(d.num_active);
    s.format = d.tree_bytes < s.need || s.need > cap;
    return s;
}

static int want_status(const InstallInputs &in)
{
    const bool device = in.engine == InstallEngine::DEVICE_INDEX, besideBuilt = in.built && !in.foreign;
    if (!in.bricks || !in.descs || in.count <= 0 || in.count > in.B) return VR_ERR_INVALID;
    if (device) {
        if (in.variant == VR_VARIANT_MIDRANGE || in.idx64) return VR_ERR_UNSUPPORTED;
        if (besideBuilt) return VR_ERR_STATE;
    }
    for (int i = 0; i < in.count; ++i) {
        if (in.bricks[i] < 0 || in.bricks[i] > in.B - 1) return VR_ERR_INVALID;
        for (int k = 0; k < i; ++k) if (in.bricks[k] == in.bricks[i]) return VR_ERR_INVALID;
        const Says s = stream_says(in.descs[i], in.maxDepth, in.treeCap);
        if (s.invalid) return VR_ERR_INVALID;
        if (s.unsupported) return VR_ERR_UNSUPPORTED;
        if (besideBuilt) return VR_ERR_STATE;       // (the host engine's place for it; the device engine never gets here)
        if (s.format) return VR_ERR_FORMAT;
    }
    return VR_OK;
}

static bool want_fine_map(const uint8_t *map, int D) { return memcmp(map + D + 1, STD_CHAIN, VR_CHAIN_LEVELS) == 0; }

static long g_plans = 0, g_checks = 0;

static void check_plan(const InstallInputs &in)
{
    const InstallPlan p = make_install_plan(in);
    const bool device = in.engine == InstallEngine::DEVICE_INDEX;
    ++g_plans;
    REQUIRE(p.status == want_status(in));
    REQUIRE(p.firstInstall == !in.built);
    REQUIRE(p.nBlk == (in.D > 12 ? (int64_t)1 << (in.D - 12) : 1));
    const bool geomFine = in.K == 6 && in.D >= 6;
    REQUIRE(p.wantFine == geomFine);
    if (p.status != VR_OK) {
        REQUIRE(p.brick.empty());
        const InstallNeeds &n = p.needs;
        REQUIRE(!n.idxTop && !n.instOff && !n.instFlag && !n.instList && !n.fineIdx && !n.idxVal3 && !n.idxBase);
        return;
    }
    REQUIRE((int)p.brick.size() == in.count);
    bool someFine = false;
    for (int i = 0; i < in.count; ++i) {
        const vr_tree_desc &d = in.descs[i];
        const InstallBrick &b = p.brick[(size_t)i];
        REQUIRE(b.need == bytes_of(d.num_active));
        REQUIRE(b.tail == (in.treeCap - b.need < 2048 ? in.treeCap - b.need : 2048) && b.tail >= 0 && b.need + b.tail <= in.treeCap);
        const bool fine = geomFine && want_fine_map(d.distance_map, in.D);
        REQUIRE(b.fineOk == fine);
        someFine = someFine || fine;
        REQUIRE(b.pass == (!device ? HostPass::BUILD_INDEX : (d.block_off ? HostPass::TABLE_CHECK : HostPass::TABLE_FROM_STREAM)));
        // never installed after a failed call: no counts are read; else exactly where the decoders' constants hold
        REQUIRE(install_fine_has(b, true) == 1 && install_fine_has(b, false) == (fine ? 1 : 0));
    }
    const InstallNeeds &n = p.needs;
    REQUIRE(n.idxTop == device && n.instOff == device && n.instFlag == device && n.instList == device);
    REQUIRE(n.fineIdx == (device ? geomFine : someFine) && n.idxVal3 == n.fineIdx);
    REQUIRE(n.idxBase == (!device && in.idx64));
}

// one entry of a call, with a violation
static void violate(int v, vr_tree_desc &d, int32_t &brick, int32_t other, int maxDepth, int64_t cap)
{
    switch (v) {
    case NULL_TREE: d.tree = nullptr; break;
    case NULL_MAP: d.distance_map = nullptr; break;
    case NULL_OFF: d.block_off = nullptr; d.top_val = g_bytes; break;
    case NULL_TOP: d.top_val = nullptr; d.block_off = g_table; break;
    case SHORT_MAP: d.map_len = maxDepth; break;
    case NA_ZERO: d.num_active = 0; break;
    case NA_MAX: d.num_active = (1ll << 32) - 1; d.tree_bytes = 1ll << 30; break;
    case NA_2P32: d.num_active = 1ll << 32; d.tree_bytes = 1ll << 30; break;
    case SHORT_BYTES: d.tree_bytes = bytes_of(d.num_active) - 1; break;
    case OVER_CAP: d.num_active = 4 * (cap + 1); d.tree_bytes = cap + 1; break;
    case AT_CAP: d.num_active = 4 * cap - 3; d.tree_bytes = cap; break;
    case TWICE: brick = other; break;
    case BRICK_B: brick = B; break;
    case BRICK_NEG: brick = -1; break;
    default: break;
    }
}

int main()
{
    const int Ds_[] = {3, 5, 6, 11, 12, 13, 20};
    const int64_t caps[] = {3000, 1ll << 31};
    const int32_t order[3][3] = {{1, 0, 0}, {2, 0, 0}, {0, 2, 1}};        // the bricks of calls of 1, 2 and 3 entries
    uint8_t stdMap[VR_MAX_DEPTH + 8];
    for (int D : Ds_) for (int kk = 0; kk < 2; ++kk) for (int64_t cap : caps) {
        InstallInputs in{};
        in.D = D; in.K = kk == 0 ? 6 : std::min(D, 4); in.Ds = std::max(D - in.K, 0); in.nIdx = (int64_t)1 << in.Ds;
        in.B = B; in.maxDepth = D + VR_CHAIN_LEVELS; in.treeCap = cap;
        for (int i = 0; i <= in.maxDepth; ++i) stdMap[i] = (uint8_t)(100 + i);
        memcpy(stdMap + D + 1, STD_CHAIN, VR_CHAIN_LEVELS);
        for (int e = 0; e < 2; ++e) for (int i64 = 0; i64 < 2; ++i64) for (int variant = 0; variant < 3; ++variant) for (int state = 0; state < 4; ++state) {
            in.engine = e ? InstallEngine::DEVICE_INDEX : InstallEngine::HOST_PARSE;
            in.idx64 = i64 != 0; in.variant = variant; in.built = (state & 1) != 0; in.foreign = (state & 2) != 0;
            for (int ci = 0; ci < 3; ++ci) for (int tables = 0; tables < 2; ++tables) {
                const int count = ci + 1;
                // a violation v0 in each entry j0 of the call; calls of two: v0 in the first entry and v1 in the second
                for (int j0 = 0; j0 < count; ++j0) for (int v0 = 0; v0 < NUM_VIOLATIONS; ++v0)
                    for (int v1 = 0; v1 < (count == 2 ? (int)NUM_VIOLATIONS : 1); ++v1) {
                        const int j1 = 1;
                        if ((count == 1 && v0 == TWICE) || (count == 2 && j0 != 0)) continue;
                        int32_t bricks[3];
                        vr_tree_desc descs[3];
                        for (int i = 0; i < count; ++i) {
                            bricks[i] = order[ci][i];
                            // streams of 37 + i tokens; a long one last, whose tail the small slots cut short
                            descs[i] = vr_tree_desc{g_bytes, 12, 37 + i, stdMap, in.maxDepth + 1, tables ? g_table : nullptr, tables ? g_bytes : nullptr};
                            if (i == count - 1) { descs[i].num_active = 4 * 2000 - 1; descs[i].tree_bytes = 2000 + i; }
                        }
                        violate(v0, descs[j0], bricks[j0], bricks[(j0 + 1) % count], in.maxDepth, cap);
                        if (count == 2) violate(v1, descs[j1], bricks[j1], bricks[(j1 + 1) % count], in.maxDepth, cap);
                        in.count = count; in.bricks = bricks; in.descs = descs;
                        snprintf(g_case, sizeof g_case, "D %d K %d cap %lld engine %d idx64 %d variant %d state %d count %d tables %d: v %d at %d, v %d at %d",
                                 D, in.K, (long long)cap, e, i64, variant, state, count, tables, v0, j0, v1, j1);
                        check_plan(in);
                    }
                // the call's own arguments
                int32_t bricks[4] = {order[ci][0], order[ci][1], order[ci][2], 0};
                vr_tree_desc descs[4];
                for (int i = 0; i < 4; ++i) descs[i] = vr_tree_desc{g_bytes, 12, 40, stdMap, in.maxDepth + 1, nullptr, nullptr};
                snprintf(g_case, sizeof g_case, "D %d K %d engine %d state %d count %d: the call's arguments", D, in.K, e, state, count);
                in.count = count; in.bricks = nullptr; in.descs = descs; check_plan(in);
                in.bricks = bricks; in.descs = nullptr; check_plan(in);
                in.descs = descs; in.count = 0; check_plan(in);
                in.count = B + 1; check_plan(in);
                // maps with one grown-branch distance off by one, in the call's last entry
                for (int lvl = 0; lvl < VR_CHAIN_LEVELS; ++lvl) for (int off = -1; off <= 1; off += 2) {
                    uint8_t map[VR_MAX_DEPTH + 8];
                    memcpy(map, stdMap, sizeof map);
                    map[D + 1 + lvl] = (uint8_t)(map[D + 1 + lvl] + off);
                    descs[count - 1].distance_map = map;
                    snprintf(g_case, sizeof g_case, "D %d K %d engine %d state %d count %d: distance %d off by %d", D, in.K, e, state, count, lvl, off);
                    in.count = count; check_plan(in);
                    REQUIRE(!std_chain_distances(map, D));
                    descs[count - 1].distance_map = stdMap;
                }
                REQUIRE(std_chain_distances(stdMap, D));
            }
        }
        // check_stream on its own: one violation, and every pair of violations in one descriptor
        for (int v0 = 0; v0 < TWICE; ++v0) for (int v1 = 0; v1 < TWICE; ++v1) {
            vr_tree_desc d{g_bytes, 12, 41, stdMap, in.maxDepth + 1, g_table, g_bytes};
            int32_t brick = 0;
            violate(v0, d, brick, 0, in.maxDepth, cap);
            violate(v1, d, brick, 0, in.maxDepth, cap);
            snprintf(g_case, sizeof g_case, "D %d cap %lld: check_stream v %d then v %d", D, (long long)cap, v0, v1);
            const StreamCheck c = check_stream(in.maxDepth, cap, d);
            const Says s = stream_says(d, in.maxDepth, cap);
            const int want = s.invalid ? VR_ERR_INVALID : (s.unsupported ? VR_ERR_UNSUPPORTED : (s.format ? VR_ERR_FORMAT : VR_OK));
            ++g_checks;
            REQUIRE(c.status == want);
            if (want == VR_OK) REQUIRE(c.need == s.need && c.tail == std::min<int64_t>(2048, cap - s.need));
            else REQUIRE(c.need == 0 && c.tail == 0);
            if (v0 == AT_CAP && v1 == NONE && cap == 3000) REQUIRE(c.status == VR_OK && c.tail == 0 && c.need == cap);
            if (v0 == OVER_CAP && v1 == NONE && cap == 3000) REQUIRE(c.status == VR_ERR_FORMAT);
            if (v0 == NA_MAX && v1 == NONE) REQUIRE(c.status == (cap >= (1ll << 30) ? VR_OK : VR_ERR_FORMAT));
            if (v0 == NA_2P32 && v1 == NONE) REQUIRE(c.status == VR_ERR_UNSUPPORTED);
        }
    }
    printf("install plans: %ld ok\n", g_plans);
    printf("stream checks: %ld ok\n", g_checks);
    return 0;
}
