// pyr12_plan_main.cpp -- which pyramid kernel a brick shape gets (volumerenderer_amd/csrc/host_plan.cpp, Pyr12Plan),
// stand-alone: tests/test_gpu_pyramid_lines.py builds it under the address and undefined-behaviour sanitizers and asks
// it for the shapes of its cases.  No device, no Python.
//   usage: pyr12_plan_main X Y Z [X Y Z ...]
//   prints, per triple:  X Y Z use12 ax ay az lines groups
// Before that it checks the rule over all 1331 power-of-two triples up to 1024: the line kernel is planned exactly
// where the bottom twelve levels split x four times (16-voxel-wide boxes) and a row holds a whole 128-byte line, and
// then the boxes of a row come in groups of eight.  The count of x splits is restated from the split rule.
#include "../volumerenderer_amd/csrc/host_plan.h"
#include <stdlib.h>

using namespace vr;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed [%lldx%lldx%lld]\n", __FILE__, __LINE__, #c, (long long)g_dims[0], (long long)g_dims[1], (long long)g_dims[2]); exit(1); } } while (0)
static int64_t g_dims[3];

// x splits among the twelve deepest levels: depth d halves axis d % 3, or the next axis still longer than one voxel
static int x_splits_bottom12(const int64_t dims[3], int D)
{
    int64_t ext[3] = {dims[0], dims[1], dims[2]};
    int n = 0;
    for (int d = 0; d < D; ++d) {
        int a = d % 3;
        for (int tries = 0; tries < 3 && ext[a] == 1; ++tries) a = (a + 1) % 3;
        ext[a] /= 2;
        if (d >= D - 12 && a == 0) ++n;
    }
    return n;
}

static Pyr12Plan plan_of(const int64_t dims[3], Geom &g)
{
    make_geom(g, dims);
    const int K = g.D < 6 ? g.D : 6;
    const int64_t heap = (int64_t)1 << (g.D + 1), numMax = heap - 1 + VR_CHAIN_LEVELS * (heap / 2);
    TilePlan t; RegionPlan r; Pyr12Plan p;
    make_plans(g, K, false, false, ((numMax + 15) / 16 + 2) * 4 + 256, t, r, p);
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) { fprintf(stderr, "usage: %s X Y Z [X Y Z ...]\n", argv[0]); return 2; }
    int planned = 0;
    for (int a = 0; a <= 10; ++a) for (int b = 0; b <= 10; ++b) for (int c = 0; c <= 10; ++c) {
        g_dims[0] = (int64_t)1 << a; g_dims[1] = (int64_t)1 << b; g_dims[2] = (int64_t)1 << c;
        Geom g;
        const Pyr12Plan p = plan_of(g_dims, g);
        const int D = a + b + c;
        const bool want = D >= 12 && x_splits_bottom12(g_dims, D) == 4 && g_dims[0] >= 128;
        REQUIRE(p.lines == want);
        if (p.lines) {
            REQUIRE(p.use12 && p.ax == 4 && p.ay + p.az == 8 && p.nbx % 8 == 0 && p.lnbx >= 3);
            REQUIRE(((int64_t)1 << (D - 12)) % 8 == 0);        // the grid: boxes / 8 groups
            ++planned;
        }
    }
    REQUIRE(planned > 0);
    printf("rule: ok, %d of 1331 triples take the line kernel\n", planned);
    for (int i = 1; i + 2 < argc; i += 3) {
        for (int k = 0; k < 3; ++k) g_dims[k] = atoll(argv[i + k]);
        for (int k = 0; k < 3; ++k) REQUIRE(g_dims[k] >= 1 && g_dims[k] <= 4096 && (g_dims[k] & (g_dims[k] - 1)) == 0);
        Geom g;
        const Pyr12Plan p = plan_of(g_dims, g);
        printf("%lld %lld %lld %d %d %d %d %d %lld\n", (long long)g_dims[0], (long long)g_dims[1], (long long)g_dims[2], (int)p.use12,
               p.use12 ? p.ax : 0, p.use12 ? p.ay : 0, p.use12 ? p.az : 0, (int)p.lines,
               p.lines ? (long long)(((int64_t)1 << (g.D - 12)) / 8) : 0ll);
    }
    return 0;
}
