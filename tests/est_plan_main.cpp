// est_plan_main.cpp -- the start-distance estimator's round plan (volumerenderer_amd/csrc/host_plan.cpp,
// est_round_plan), stand-alone: tests/test_est_round_plan.py builds it under the address and undefined-behaviour
// sanitizers.  No device, no Python.
//   usage: est_plan_main [LEVEL ...]
// Checks, for every level of 2^13 .. 2^31 nodes and both schedules, what k_est_summ and k_est_walk rely on: the rounds
// start behind the four head segments, their limits increase strictly until one reaches the level's end (no round
// without segments of its own) and stay there, the level's end is reached no later than the last-but-one round, the last
// round is an exact one, and no window is empty or wider than a record.  Then the window rule: a window holds its own
// threshold and stays inside [0, 256).  Prints the plan of every LEVEL given:  LEVEL schedule nseg  segEnd:nc:kernel ...
#include "../volumerenderer_amd/csrc/host_plan.h"
#include <stdlib.h>

using namespace vr;

static int g_level, g_old;
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed [level %d, old schedule %d]\n", __FILE__, __LINE__, #c, g_level, g_old); exit(1); } } while (0)

int main(int argc, char **argv)
{
    const uint32_t first = VR_EST_HEAD / VR_EST_SEG;
    for (g_old = 0; g_old <= 1; ++g_old)
        for (g_level = 13; g_level <= 31; ++g_level) {
            const uint32_t nseg = (uint32_t)(((uint64_t)1 << g_level) / VR_EST_SEG);
            const EstPlan p = est_round_plan(nseg, g_old != 0);
            REQUIRE(p.rounds >= 2 && p.rounds <= VR_EST_MAX_ROUNDS);
            uint32_t at = first;
            for (int r = 0; r < p.rounds; ++r) {
                const EstRound &R = p.r[r];
                REQUIRE(R.nc >= 1 && R.nc <= VR_EST_CAND);
                REQUIRE(R.sweeps >= 1);
                REQUIRE(R.segEnd > first && R.segEnd <= nseg);
                if (at < nseg) REQUIRE(R.segEnd > at);          // strictly increasing up to the level's end
                else REQUIRE(R.segEnd == nseg);
                if (g_old) REQUIRE(R.segEnd == nseg);
                at = R.segEnd;
            }
            REQUIRE(p.r[p.rounds - 2].segEnd == nseg);
            REQUIRE(!p.r[p.rounds - 1].quads && p.r[p.rounds - 1].nc == VR_EST_CAND);
            if (g_old) REQUIRE(p.rounds == 5 && p.r[0].quads && p.r[0].nc == 4 && !p.r[1].quads && p.r[1].nc == 4 && p.r[2].nc == VR_EST_CAND);
        }
    g_level = 12; g_old = 0;
    REQUIRE(est_round_plan(first, false).rounds == 0 && est_round_plan(first, true).rounds == 0);      // the head is the whole level
    for (int nc = 1; nc <= VR_EST_CAND; ++nc)
        for (int up = 0; up <= 1; ++up)
            for (int T = 0; T < 256; ++T) {
                const int b = est_window_base(T, up, nc);
                REQUIRE(b >= 0 && b + nc <= 256 && b <= T && T < b + nc);
                if (nc == 4 && T >= 1 && T <= 253) REQUIRE(b == T - 1);
                if (nc == 8 && T >= 2 && T <= 250) REQUIRE(b == T - 2);
                if (nc == 2 && T >= 1 && T <= 254) REQUIRE(b == (up ? T : T - 1));
            }
    printf("rule: ok\n");
    for (int i = 1; i < argc; ++i) {
        const int level = atoi(argv[i]);
        if (level < 13 || level > 31) { fprintf(stderr, "level %d outside 13 .. 31\n", level); return 2; }
        for (int old = 0; old <= 1; ++old) {
            const uint32_t nseg = (uint32_t)(((uint64_t)1 << level) / VR_EST_SEG);
            const EstPlan p = est_round_plan(nseg, old != 0);
            printf("%d %s %u ", level, old ? "old" : "new", nseg);
            for (int r = 0; r < p.rounds; ++r) printf(" %u:%d:%c", p.r[r].segEnd, p.r[r].nc, p.r[r].quads ? 'q' : 'x');
            printf("\n");
        }
    }
    return 0;
}
