// build_plan_main.cpp -- the plan of a build and the switch table (volumerenderer_amd/csrc/host_plan.cpp:
// make_build_plan, build_level, build_side_streams, VR_SWITCHES), stand-alone: tests/test_build_plan.py builds it under
// the address and undefined-behaviour sanitizers.  No device, no Python.
//   usage: build_plan_main
// Restates the rules of vr_brickset_build in its own words -- it calls nothing of the unit but the functions under
// test -- and compares every field of the plan over the cross product of
//   D 0 1 9 10 11 12 13 14 15 16 22 23 28; k_pyramid12 on / off from D 12, its lines form on / off from D 15;
//   the three variants; epochs 0 1 2; tolerance 0 1; B 1 31 32 33 63 64; 1 .. 4 level-loop streams with 0 .. 3 side
//   streams; every build switch on and off (all 64 combinations with 1 stream / no side stream and with 4 / 3, none
//   and all of them at the other stream settings); compaction on and off; general extents on and off
// and every level of those plans (for two B and two stream settings: a level does not depend on them).  Per case also:
// the brick ranges tile [0, B); the pyramid's rounds sum to D (D - 12 behind k_pyramid12); a level's fill grid covers
// it; uniformBlocks => skipBlocks => fused.  Then the switch table: every row is found by its name and by no other, an
// unknown name is refused, the environment names are the rows' in capitals.  Prints "plans: <n> ok", then one line
// "switch <name> <ENV>" per row.
#include "../volumerenderer_amd/csrc/host_plan.h"
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>

using namespace vr;

static char g_case[256];
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_case); exit(1); } } while (0)

static int64_t up(int64_t a, int64_t b) { return (a + b - 1) / b; }
static int64_t p2(int e) { return (int64_t)1 << (e < 0 ? 0 : e); }

static void check_level(const BuildInputs &in, const BuildPlan &p, int d)
{
    const BuildLevel l = build_level(p, d);
    const int D = in.D;
    const int64_t n = (int64_t)1 << d;
    const bool big = D >= 12;
    const bool skip = big && in.use12 && in.tolerance > 0 && in.maxEpochs > 0 && D >= 14 && !in.sw.noSkipBlocks;
    REQUIRE(l.constLeaves == (skip && d + 1 == D));
    if (n <= 4096) REQUIRE(l.est.rounds == 0);
    else {
        const EstPlan e = est_round_plan((uint32_t)(n / 1024), in.sw.estOldSchedule);
        REQUIRE(l.est.rounds == e.rounds && e.rounds >= 2);
        for (int r = 0; r < e.rounds; ++r) {
            REQUIRE(l.est.r[r].segEnd == e.r[r].segEnd && l.est.r[r].nc == e.r[r].nc && l.est.r[r].quads == e.r[r].quads && l.est.r[r].sweeps == e.r[r].sweeps);
            const int64_t segs = (int64_t)e.r[r].segEnd - 4;      // behind the four head segments
            const bool byteQuads = e.r[r].quads && !in.sw.estExactBounds;
            int64_t gx = e.r[r].quads ? up(segs, 8 * (int64_t)e.r[r].sweeps) : up(segs, 8);
            if (!e.r[r].quads && gx > 64) gx = 64;
            REQUIRE(l.estL[r].gx == (uint32_t)gx && gx >= 1);
            REQUIRE(l.estL[r].quads == byteQuads);
            REQUIRE(l.estL[r].budget == (byteQuads ? in.sw.estBudget : -1));
        }
    }
    const bool leafLevelKeptOut = big && in.maxEpochs > 0 && d == D;
    REQUIRE(l.sumsOnly == leafLevelKeptOut);
    if (n < 4096) {
        REQUIRE(!l.fill16 && l.fillGrid == (uint32_t)up(n, 1024));
        REQUIRE((int64_t)l.fillGrid * FILL_NODES_PER_BLOCK >= n);
    } else {
        const int64_t chunks = n / 4096;
        const int iters = chunks >= 512 ? 8 : (chunks >= 64 ? 4 : 1);
        REQUIRE(l.fill16 && l.iters == iters && l.fillGrid == (uint32_t)up(chunks, iters));
        REQUIRE((int64_t)l.fillGrid * l.iters * 4096 >= n && l.iters <= FILL_ITERS);
    }
}

static void check_plan(const BuildInputs &in, bool levels)
{
    snprintf(g_case, sizeof(g_case), "D %d B %d variant %d tol %d epochs %d use12 %d lines %d general %d streams %d side %d compact %d sw %d%d%d%d%d%d",
             in.D, in.B, in.variant, in.tolerance, in.maxEpochs, in.use12, in.lines, in.generalGeom, in.levelLoopStreams, in.sideStreams,
             in.compactOnBuild, in.sw.noSkipBlocks, in.sw.noUniformBlocks, in.sw.pyramidBoxes, in.sw.indexPerBlock, in.sw.estExactBounds, in.sw.estOldSchedule);
    const BuildPlan p = make_build_plan(in);
    const int D = in.D, B = in.B;
    const bool mr = in.variant == 2, big = D >= 12, loop = in.maxEpochs > 0;
    REQUIRE(p.D == D && p.B == B && p.maxEpochs == in.maxEpochs);
    REQUIRE(p.midRange == mr && p.guarded == (in.variant == 1 || in.variant == 2));
    REQUIRE(p.fused == big);
    REQUIRE(p.leafless == (big && loop));
    const bool skip = big && in.use12 && in.tolerance > 0 && loop && D >= 14 && !in.sw.noSkipBlocks;
    REQUIRE(p.skipBlocks == skip);
    REQUIRE(p.constClosedForm == (loop && in.tolerance > 0 && D > 0));
    REQUIRE(p.zeroFill == !loop);
    REQUIRE(p.boxes == p2(D - 12));
    // pyramid
    REQUIRE(p.pyr12 == in.use12);
    const bool lines = in.use12 && in.lines && !in.sw.pyramidBoxes;
    REQUIRE(p.pyr12Lines == lines);
    if (in.use12) REQUIRE(p.pyr12Grid == (uint32_t)(lines ? p2(D - 15) : p2(D - 12)) && (lines ? D >= 15 : D >= 12));
    REQUIRE(p.pyrSrcIdx == (!in.use12 && in.generalGeom));
    int at = in.use12 ? D - 12 : D, sum = 0;
    REQUIRE(p.pyrRounds >= (in.use12 ? 0 : 1) && p.pyrRounds <= VR_PYR_MAX_ROUNDS);
    for (int r = 0; r < p.pyrRounds; ++r) {
        const int L = at > 10 ? 10 : at;
        REQUIRE(p.pyr[r].dLeaf == at && p.pyr[r].L == L && p.pyr[r].blocks == (uint32_t)p2(at - L));
        REQUIRE(L > 0 || (r == 0 && D == 0));
        at -= L; sum += L;
    }
    REQUIRE(at == 0 && sum == (in.use12 ? D - 12 : D));
    REQUIRE(p.rootStride == p2(D - 10));
    // level-loop split
    const int want = in.levelLoopStreams < 4 ? in.levelLoopStreams : 4;
    int parts = 1;
    if (!mr && B >= 16 * want && want >= 2) parts = want < 1 + in.sideStreams ? want : 1 + in.sideStreams;
    REQUIRE(p.parts == parts && parts >= 1 && parts <= VR_MAX_PARTS);
    REQUIRE(p.range[0] == 0 && p.range[parts] == B);
    for (int i = 0; i < parts; ++i) {
        REQUIRE(p.range[i] == (int32_t)((int64_t)B * i / parts));
        REQUIRE(p.range[i] < p.range[i + 1]);        // no gap, no overlap, no empty range
    }
    REQUIRE(p.forkRange == (mr && in.sideStreams > 0));
    const int side = build_side_streams(in.variant, B, in.levelLoopStreams);
    REQUIRE(side == (mr ? 1 : ((B >= 16 * want && want >= 2) ? want - 1 : 0)));
    REQUIRE(parts <= 1 + side && (!p.forkRange || side == 1));     // a build never uses a stream it did not ask for
    REQUIRE(p.estOldSchedule == in.sw.estOldSchedule && p.estExactBounds == in.sw.estExactBounds && p.estBudget == in.sw.estBudget);
    // prune
    const bool uniform = skip && !mr && !in.sw.noUniformBlocks;      // (skip implies a leafless build)
    REQUIRE(p.uniformBlocks == uniform);
    REQUIRE(!p.uniformBlocks || p.skipBlocks);
    REQUIRE(!p.skipBlocks || (p.fused && p.leafless));
    if (big) REQUIRE(p.uniformGrid == (uint32_t)up(p2(D - 12), 16) && p.pruneGrid == (uint32_t)p2(D - 12));
    else REQUIRE(p.pruneGrid == (uint32_t)up(p2(D), 256));
    REQUIRE(p.pruneFrom == (big ? D - 13 : D - 1));
    // convert
    REQUIRE(p.emitLeaves == (big ? 4096 : 256));
    REQUIRE(p.nblk == up(p2(D), big ? 4096 : 256));
    const int64_t nIdx = p2(D < 6 ? 0 : D - 6);
    if (big && !in.sw.indexPerBlock) {
        REQUIRE(p.index == VR_INDEX12 && p.indexGrid == (uint32_t)up(p.nblk, 32));
        REQUIRE(p.constFinishGrid == 1 && p.constFinishThreads == 64 && p.constFinishIdx == 0);
    } else {
        if (big) REQUIRE(p.index == VR_INDEX12_BLOCK && p.indexGrid == (uint32_t)up(p.nblk, 4));
        else REQUIRE(p.index == VR_EMIT_WRITE && p.indexGrid == (uint32_t)p.nblk);
        REQUIRE(p.constFinishGrid == (uint32_t)up(nIdx, 256) && p.constFinishThreads == 256 && p.constFinishIdx == nIdx);
    }
    REQUIRE(p.statRecords == up(p2(D), big ? 1024 : 256));
    REQUIRE(p.gapped == big && p.compact == (big && in.compactOnBuild));
    REQUIRE(build_fused(D) == big);
    if (levels) for (int d = 0; d <= D; ++d) check_level(in, p, d);
}

int main()
{
    const int Ds[] = {0, 1, 9, 10, 11, 12, 13, 14, 15, 16, 22, 23, 28}, Bs[] = {1, 31, 32, 33, 63, 64};
    long cases = 0;
    for (const int D : Ds)
        for (int pyr = 0; pyr < 3; ++pyr) {          // 0: rounds only, 1: k_pyramid12, 2: its lines form applies
            if ((pyr >= 1 && D < 12) || (pyr == 2 && D < 15)) continue;
            for (int variant = 0; variant <= 2; ++variant)
                for (int epochs = 0; epochs <= 2; ++epochs)
                    for (int tol = 0; tol <= 1; ++tol)
                        for (const int B : Bs)
                            for (int streams = 1; streams <= 4; ++streams)
                                for (int side = 0; side <= 3; ++side)
                                    for (int sw = 0; sw < 64; ++sw)
                                        for (int cg = 0; cg < 4; ++cg) {
                                            // (every switch combination at the two extreme stream settings; none and all at the others)
                                            if (streams + side != 1 && streams + side != 7 && sw != 0 && sw != 63) continue;
                                            BuildInputs in{};
                                            in.D = D; in.B = B; in.variant = variant; in.tolerance = tol; in.maxEpochs = epochs;
                                            in.use12 = pyr >= 1; in.lines = pyr == 2; in.generalGeom = (cg & 2) != 0;
                                            in.sw.noSkipBlocks = sw & 1; in.sw.noUniformBlocks = sw & 2; in.sw.pyramidBoxes = sw & 4;
                                            in.sw.indexPerBlock = sw & 8; in.sw.estExactBounds = sw & 16; in.sw.estOldSchedule = sw & 32;
                                            in.sw.estBudget = (sw & 16) ? 3 : EST_QUAD_BUDGET;
                                            in.levelLoopStreams = streams; in.compactOnBuild = (cg & 1) != 0; in.sideStreams = side;
                                            check_plan(in, (B == 1 || B == 33) && streams + side == (B == 1 ? 1 : 7));
                                            ++cases;
                                        }
        }
    printf("plans: %ld ok\n", cases);
    // ---- the switch table
    snprintf(g_case, sizeof(g_case), "switch table");
    REQUIRE(VR_NUM_SWITCHES >= 1);
    std::set<std::string> names;
    for (int i = 0; i < VR_NUM_SWITCHES; ++i) {
        const SwitchRow &row = VR_SWITCHES[i];
        REQUIRE(row.name && row.member && names.insert(row.name).second);
        REQUIRE(find_switch(row.name) == row.member);
        for (int j = 0; j < i; ++j) REQUIRE(VR_SWITCHES[j].member != row.member);      // no two names for one switch
        // setting it through the table sets that member and no other
        Switches w;
        w.*find_switch(row.name) = true;
        int on = 0;
        for (int j = 0; j < VR_NUM_SWITCHES; ++j) on += w.*VR_SWITCHES[j].member ? 1 : 0;
        REQUIRE(on == 1 && w.*row.member && w.estBudget == EST_QUAD_BUDGET);
        char env[64];
        switch_env_name(row.name, env, sizeof(env));
        std::string want = "VRHIP_";
        for (const char *c = row.name; *c; ++c) want += (char)(*c >= 'a' && *c <= 'z' ? *c - 32 : *c);
        REQUIRE(want == env);
        printf("switch %s %s\n", row.name, env);
    }
    REQUIRE(!find_switch("no_such_switch") && !find_switch("") && !find_switch(nullptr) && !find_switch("decode_wal") && !find_switch("DECODE_WALK"));
    REQUIRE(!find_switch("est_budget"));      // an integer, from the environment only
    // create-time: exactly the rows whose variable is set, and the budget's integer
    for (int i = 0; i < VR_NUM_SWITCHES; ++i) {
        char env[64];
        switch_env_name(VR_SWITCHES[i].name, env, sizeof(env));
        unsetenv(env);
    }
    unsetenv("VRHIP_EST_BUDGET");
    Switches none = switches_from_env();
    for (int j = 0; j < VR_NUM_SWITCHES; ++j) REQUIRE(!(none.*VR_SWITCHES[j].member));
    REQUIRE(none.estBudget == EST_QUAD_BUDGET);
    for (int i = 0; i < VR_NUM_SWITCHES; ++i) {
        char env[64];
        switch_env_name(VR_SWITCHES[i].name, env, sizeof(env));
        setenv(env, "1", 1);
        setenv("VRHIP_EST_BUDGET", i & 1 ? "-5" : "17", 1);
        const Switches w = switches_from_env();
        for (int j = 0; j < VR_NUM_SWITCHES; ++j) REQUIRE((w.*VR_SWITCHES[j].member) == (j == i));
        REQUIRE(w.estBudget == (i & 1 ? EST_QUAD_BUDGET : 17));
        unsetenv(env);
    }
    printf("switches: %d ok\n", VR_NUM_SWITCHES);
    return 0;
}
