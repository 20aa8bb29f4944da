// host_plan_main.cpp -- stand-alone checks of volumerenderer_amd/csrc/host_plan.{h,cpp} (tests/test_host_plan.py builds
// it with the address and undefined-behaviour sanitizers and runs it).  No device, no Python.  Everything is checked
// by definition (restated here, sharing no code with the unit) except the tile / region launch plans, whose meaning
// only the kernels define: those are compared with tests/golden/decode_plans.json.
//   usage: host_plan_main <golden tree file> <decode_plans.json>
#include "../volumerenderer_amd/csrc/host_plan.h"
#include <stdlib.h>
#include <string.h>
#include <string>

using namespace vr;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_ctx.c_str()); exit(1); } } while (0)
static std::string g_ctx;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;      // fixed seed: every run checks the same cases
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

static int ilog2(int64_t v) { int n = 0; while (((int64_t)1 << (n + 1)) <= v) ++n; return n; }

// ---- geometry ------------------------------------------------------------------------------------------------------
// buildRecursive's rule as a walk over one box: depth d halves axis d % 3, or the next axis that is still longer than
// one voxel; the half a voxel falls into is decided by the coordinate bit log2(extent / 2)
static void naive_splits(const int64_t dims[3], int D, int axis[], int bit[])
{
    int64_t lo[3] = {0, 0, 0}, hi[3] = {dims[0], dims[1], dims[2]};
    for (int d = 0; d < D; ++d) {
        int a = d % 3;
        for (int tries = 0; tries < 3 && hi[a] - lo[a] == 1; ++tries) a = (a + 1) % 3;
        const int64_t mid = (lo[a] + hi[a]) / 2;
        axis[d] = a; bit[d] = ilog2(mid - lo[a]);
        hi[a] = mid;
    }
}

struct Fixture { std::vector<long long> v; size_t at = 0; long long next() { REQUIRE(at < v.size()); return v[at++]; } };

static void check_geometry(Fixture &fx)
{
    for (int a = 0; a <= 10; ++a) for (int b = 0; b <= 10; ++b) for (int c = 0; c <= 10; ++c) {
        const int64_t dims[3] = {(int64_t)1 << a, (int64_t)1 << b, (int64_t)1 << c};
        g_ctx = std::to_string(dims[0]) + "x" + std::to_string(dims[1]) + "x" + std::to_string(dims[2]);
        Geom g;
        make_geom(g, dims);
        const int D = a + b + c;
        REQUIRE(g.D == D && g.X == dims[0] && g.Y == dims[1] && g.Z == dims[2] && g.voxels == dims[0] * dims[1] * dims[2]);
        REQUIRE(g.nb[0] == a && g.nb[1] == b && g.nb[2] == c);
        int axis[32], bit[32];
        naive_splits(dims, D, axis, bit);
        for (int d = 0; d < D; ++d) REQUIRE(g.axis[d] == axis[d] && g.bit[d] == bit[d]);
        // split counts
        const std::vector<std::array<int, 3>> sc = split_counts(dims, D);
        REQUIRE((int)sc.size() == D + 1);
        int n[3] = {0, 0, 0};
        for (int d = 0; d <= D; ++d) {
            for (int k = 0; k < 3; ++k) REQUIRE(sc[(size_t)d][(size_t)k] == n[k]);
            if (d < D) ++n[axis[d]];
        }
        // rank_to_xyz is a bijection: it ORs one coordinate bit per set rank bit (OR-linear in the rank bits: its loop
        // over the depths), so it is one exactly if the D unit ranks hit D distinct coordinate bits (checked for all
        // triples; above 2^15 voxels the check rests on this plus the 4096 sampled round trips); small triples are enumerated
        const std::vector<uint32_t> sp = make_spread(g);
        REQUIRE((int64_t)sp.size() == dims[0] + dims[1] + dims[2]);
        const auto rank_of = [&](int x, int y, int z) { return sp[(size_t)x] | sp[(size_t)(g.X + y)] | sp[(size_t)(g.X + g.Y + z)]; };
        uint32_t seen[3] = {0, 0, 0};
        for (int k = 0; k < D; ++k) {
            int p[3];
            rank_to_xyz(g, 1u << k, p[0], p[1], p[2]);
            int nz = 0;
            for (int q = 0; q < 3; ++q) if (p[q]) { ++nz; REQUIRE((p[q] & (p[q] - 1)) == 0 && !(seen[q] & (uint32_t)p[q])); seen[q] |= (uint32_t)p[q]; }
            REQUIRE(nz == 1);
        }
        REQUIRE(seen[0] == g.X - 1u && seen[1] == g.Y - 1u && seen[2] == g.Z - 1u);
        const bool small = D <= 15;
        std::vector<uint8_t> hit(small ? (size_t)g.voxels : 0, 0);
        for (int64_t i = 0; i < (small ? g.voxels : 4096); ++i) {
            // spread is the inverse: every voxel of the small triples, 4096 sampled voxels of the others
            const int64_t v = small ? i : (int64_t)((((uint64_t)rnd() << 31) ^ rnd()) % (uint64_t)g.voxels);
            const int x = (int)(v % g.X), y = (int)((v / g.X) % g.Y), z = (int)(v / ((int64_t)g.X * g.Y));
            const uint32_t r = rank_of(x, y, z);
            REQUIRE((uint64_t)r < ((uint64_t)1 << D));
            int rx, ry, rz;
            rank_to_xyz(g, r, rx, ry, rz);
            REQUIRE(rx == x && ry == y && rz == z);
            if (small) {
                rank_to_xyz(g, (uint32_t)i, rx, ry, rz);
                REQUIRE(rx >= 0 && rx < g.X && ry >= 0 && ry < g.Y && rz >= 0 && rz < g.Z);
                uint8_t &h = hit[(size_t)rx + (size_t)g.X * ((size_t)ry + (size_t)g.Y * (size_t)rz)];
                REQUIRE(!h);
                h = 1;
            }
        }
        // make_lut: the voxel of local rank lr of a depth-(D-K) subtree, relative to the subtree's first voxel
        const int K = D < 6 ? D : 6;
        const std::vector<uint32_t> lut = make_lut(g, K);
        REQUIRE(lut.size() == (size_t)1 << K);
        const uint32_t roots[3] = {0u, (uint32_t)(((uint64_t)1 << (D - K)) - 1), (uint32_t)(rnd() % ((uint64_t)1 << (D - K)))};
        for (uint32_t s : roots)
            for (uint32_t lr = 0; lr < (1u << K); ++lr) {
                int ox, oy, oz, x, y, z;
                rank_to_xyz(g, s << K, ox, oy, oz);
                rank_to_xyz(g, (s << K) | lr, x, y, z);
                REQUIRE(lut[lr] == ((uint32_t)(x - ox) | ((uint32_t)(y - oy) << 10) | ((uint32_t)(z - oz) << 20)));
            }
        // the plans
        const int64_t heap = (int64_t)1 << (D + 1), numMax = heap - 1 + VR_CHAIN_LEVELS * (heap / 2);
        int64_t treeCap = ((numMax + 15) / 16 + 2) * 4 + 256;       // as vr_brickset_create sizes the stream buffer
        if (D >= 12 && ((int64_t)1 << (D - 12)) * 2320 * 4 + 256 > treeCap) treeCap = ((int64_t)1 << (D - 12)) * 2320 * 4 + 256;
        TilePlan t; RegionPlan r; Pyr12Plan p;
        make_plans(g, K, false, false, treeCap, t, r, p);
        int nx12 = 0;
        for (int d = D - 12; d >= 0 && d < D; ++d) nx12 += axis[d] == 0;
        REQUIRE(p.use12 == (D >= 12 && nx12 >= 4));
        if (p.use12) {
            REQUIRE(p.ax + p.ay + p.az == 12 && p.ax == nx12);
            for (int i = 0; i < 16; ++i) {
                uint32_t want = 0;
                for (int d = D - 12; d < D; ++d) if (axis[d] == 0) want |= (uint32_t)((i >> bit[d]) & 1) << (D - 1 - d);
                REQUIRE(p.sx[i] == want);
            }
            REQUIRE(p.nbx == (g.X >> p.ax) && p.nby == (g.Y >> p.ay) && (1 << p.lnbx) == p.nbx && (1 << p.lnby) == p.nby);
        }
        // ... tile and region: field by field against the fixture (recorded from the code before the plans moved here)
        REQUIRE(fx.next() == dims[0] && fx.next() == dims[1] && fx.next() == dims[2]);
        const long long tv[9] = {t.ok, t.jx, t.jy, t.jz, t.tilesX, t.tilesY, t.tilesZ, t.ltx, t.lty};
        for (long long f : tv) REQUIRE(fx.next() == f);
        for (int i = 0; i < 8; ++i) REQUIRE(fx.next() == t.kqBit[i]);
        const long long rv[8] = {r.ok, r.X, r.Y, (long long)r.voxels, r.lrx, r.lry, r.jx, r.lanePos};
        for (long long f : rv) REQUIRE(fx.next() == f);
        for (int i = 0; i < 4; ++i) REQUIRE(fx.next() == r.parkP[i]);
        REQUIRE(fx.next() == r.parkS);
        for (int i = 0; i < 4; ++i) REQUIRE(fx.next() == r.gAddr[i]);
        REQUIRE(fx.next() == r.gByte);
        for (int i = 0; i < 8; ++i) REQUIRE(fx.next() == r.gOut[i]);
        const long long re[6] = {r.xRead[0], r.xRead[1], r.blkX, r.blkY, r.blkZ, r.nreg};
        for (long long f : re) REQUIRE(fx.next() == f);
    }
    REQUIRE(fx.at == fx.v.size());
    g_ctx.clear();
}

// ---- the stream walker ---------------------------------------------------------------------------------------------
struct Stream { int D; std::vector<uint8_t> tok; uint8_t dmap[VR_MAX_DEPTH + 8]; };

static std::vector<uint8_t> pack(const std::vector<uint8_t> &tok, size_t n)     // TwoBitArray packing, exactly (n + 3) / 4 bytes
{
    std::vector<uint8_t> b((n + 3) / 4, 0);
    for (size_t i = 0; i < n; ++i) b[i / 4] |= (uint8_t)((i < tok.size() ? tok[i] : 0) << (2 * (i % 4)));
    return b;
}

// a grammatical stream: subtree := 3 | code subtree subtree (above the leaves) | code branch (a leaf);
// branch := up to seven codes, ended by a 3 unless all seven are there
static void gen_subtree(Stream &s, int j, uint32_t prunePermille)
{
    if (rnd() % 1000 < prunePermille) { s.tok.push_back(3); return; }
    s.tok.push_back((uint8_t)(rnd() % 3));
    if (j < s.D) { gen_subtree(s, j + 1, prunePermille); gen_subtree(s, j + 1, prunePermille); return; }
    const int len = (int)(rnd() % 8);
    for (int c = 0; c < len; ++c) s.tok.push_back((uint8_t)(rnd() % 3));
    if (len < VR_CHAIN_LEVELS) s.tok.push_back(3);
}

// The naive decoder: one function per grammar rule, recursion instead of a stack, vectors indexed by the node's path.
struct Naive {
    const Stream &s;
    int Ds, cut;
    size_t pos = 0;
    std::vector<uint32_t> offs;
    std::vector<uint8_t> vals, val3, fine;      // fine: tokens per group of four leaves, by the group's number
    Naive(const Stream &st, int ds, int ct) : s(st), Ds(ds), cut(ct), offs((size_t)1 << ds, VR_IDX_DEAD), vals((size_t)1 << ds, 0),
        val3(st.D >= 6 ? (size_t)1 << (st.D - 3) : 0, 0), fine(st.D >= 6 ? (size_t)1 << (st.D - 2) : 0, 0) {}
    void count(int j, uint32_t path) { if (j >= Ds && !fine.empty()) ++fine[(size_t)(path << (s.D - j)) >> 2]; }
    void fill(int j, uint32_t path, int val)     // a pruned node stands for every node below it
    {
        if (j == Ds) vals[path] = (uint8_t)val;
        if (j == s.D - 3 && !val3.empty()) val3[path] = (uint8_t)val;
        if (j < Ds || j < s.D - 3) { fill(j + 1, 2 * path, val); fill(j + 1, 2 * path + 1, val); }
    }
    void branch(uint32_t leaf)
    {
        for (int c = 0; c < VR_CHAIN_LEVELS; ++c) { count(s.D, leaf); if (s.tok[pos++] == 3) return; }
    }
    void subtree(int j, uint32_t path, int parent)
    {
        const int tok = s.tok[pos];
        int val = parent;
        if (j == 0) val = s.dmap[0];
        else if (j <= cut && tok == 1) val = parent + s.dmap[j] > 255 ? 255 : parent + s.dmap[j];
        else if (j <= cut && tok == 2) val = parent - s.dmap[j] < 0 ? 0 : parent - s.dmap[j];
        if (j == Ds) offs[path] = (uint32_t)pos;
        count(j, path);
        ++pos;
        if (tok == 3) { fill(j, path, val); return; }
        if (j == Ds) vals[path] = (uint8_t)val;
        if (j == s.D - 3 && !val3.empty()) val3[path] = (uint8_t)val;
        if (j == s.D) { branch(path); return; }
        subtree(j + 1, 2 * path, val);
        subtree(j + 1, 2 * path + 1, val);
    }
};

static void check_walker(const Stream &s)
{
    const int D = s.D, K = D < 6 ? D : 6, Ds = D - K;
    const int64_t nIdx = (int64_t)1 << Ds, n = (int64_t)s.tok.size();
    const std::vector<uint8_t> bytes = pack(s.tok, s.tok.size());
    std::vector<uint32_t> offs;
    std::vector<uint8_t> vals, fine, val3;
    REQUIRE(build_index_from_stream(D, Ds, K, nIdx, bytes.data(), n, s.dmap, offs, vals, fine, val3) == 0);
    Naive full(s, Ds, D);
    full.subtree(0, 0, 0);
    REQUIRE(full.pos == s.tok.size());
    REQUIRE(offs == full.offs && vals == full.vals && val3 == full.val3);
    // the unit keeps the counts 16 per depth-Ds node: group (first leaf >> 2) = node * 16 + group in the node
    REQUIRE(fine == full.fine);
    for (int cut = 0; cut < Ds; ++cut) {
        std::vector<uint8_t> cv;
        REQUIRE(cut_values_from_stream(D, Ds, K, nIdx, bytes.data(), n, s.dmap, cut, cv) == 0);
        Naive part(s, Ds, cut);
        part.subtree(0, 0, 0);
        REQUIRE(cv == part.vals);
    }
}

// Malformed input: a definite return code (0 or negative) and no access outside the (numActive + 3) / 4 bytes handed
// over -- the copy is a heap block of exactly that size, so the address sanitizer sees any over-read.  How many
// mutants are rejected is not bounded more tightly than "at most all of them": a flipped token often leaves a
// grammatical stream.  The unmutated stream must be accepted (check_walker).
static int run_both(const Stream &s, const std::vector<uint8_t> &tok, size_t numActive)
{
    const int D = s.D, K = D < 6 ? D : 6, Ds = D - K;
    const std::vector<uint8_t> packed = pack(tok, numActive);
    uint8_t *exact = (uint8_t *)malloc(packed.size() ? packed.size() : 1);
    REQUIRE(exact);
    if (!packed.empty()) memcpy(exact, packed.data(), packed.size());
    std::vector<uint32_t> offs;
    std::vector<uint8_t> vals, fine, val3, cv;
    const int a = build_index_from_stream(D, Ds, K, (int64_t)1 << Ds, exact, (int64_t)numActive, s.dmap, offs, vals, fine, val3);
    const int b = cut_values_from_stream(D, Ds, K, (int64_t)1 << Ds, exact, (int64_t)numActive, s.dmap, Ds / 2, cv);
    free(exact);
    REQUIRE(a <= 0 && a >= -3 && b <= 0 && b >= -3);
    REQUIRE((a == 0) == (b == 0));      // one grammar
    return a;
}

static void check_malformed(const Stream &s)
{
    int total = 0, rejected = 0;
    const size_t n = s.tok.size();
    for (size_t k = 1; k <= 64 && k <= n; ++k) { ++total; rejected += run_both(s, s.tok, n - k) != 0; }
    for (size_t k = 1; k <= 8; ++k) { ++total; rejected += run_both(s, s.tok, n + k) != 0; }
    std::vector<uint8_t> tok = s.tok;
    for (int m = 0; m < 2000; ++m) {
        const size_t at = rnd() % n;
        const uint8_t old = tok[at];
        tok[at] = (uint8_t)((old + 1 + rnd() % 3) & 3);
        ++total; rejected += run_both(s, tok, n) != 0;
        tok[at] = old;
    }
    REQUIRE(rejected >= 0 && rejected <= total);
    printf("  D=%d, %zu tokens: %d of %d malformed variants rejected\n", s.D, n, rejected, total);
}

// ---- the file header -----------------------------------------------------------------------------------------------
static bool reread(const void *bytes, size_t n, Header &h)
{
    FILE *f = tmpfile();
    REQUIRE(f);
    REQUIRE(fwrite(bytes, 1, n, f) == n);
    rewind(f);
    const bool ok = read_header(f, h);
    fclose(f);
    return ok;
}

static void check_header()
{
    const Header h = {{0, 0, 0}, {64, 32, 16}, 22, 15, 64, 32, 16, 12345};
    FILE *f = tmpfile();
    REQUIRE(f && write_header(f, h));
    REQUIRE(ftell(f) == VR_HEADER_BYTES);
    rewind(f);
    uint8_t raw[VR_HEADER_BYTES];
    REQUIRE(fread(raw, 1, sizeof(raw), f) == sizeof(raw));
    fclose(f);
    // the layout of the reference's save(): six int64, two int32, four int64, little endian
    const auto i64 = [&](int at) { long long v = 0; for (int i = 7; i >= 0; --i) v = (v << 8) | raw[at + i]; return v; };
    REQUIRE(i64(24) == 64 && i64(32) == 32 && i64(40) == 16 && (i64(48) & 0xFFFFFFFF) == 22 && (i64(48) >> 32) == 15);
    REQUIRE(i64(56) == 64 && i64(64) == 32 && i64(72) == 16 && i64(80) == 12345);
    Header back;
    REQUIRE(reread(raw, sizeof(raw), back) && memcmp(&back, &h, sizeof(h)) == 0);
    REQUIRE(!reread(raw, sizeof(raw) - 1, back));
    REQUIRE(!reread(raw, 0, back));
    for (int mtd : {-1, 0, VR_CHAIN_LEVELS - 1, VR_MAX_DEPTH, VR_MAX_DEPTH + 1, 1 << 30}) { Header bad = h; bad.maxDepth = mtd; REQUIRE(!reread(&bad, sizeof(bad), back)); }
    for (int mtd : {VR_CHAIN_LEVELS, VR_MAX_DEPTH - 1}) { Header good = h; good.maxDepth = mtd; REQUIRE(reread(&good, sizeof(good), back)); }
    for (long long na : {0ll, -1ll, -(1ll << 40)}) { Header bad = h; bad.numActive = na; REQUIRE(!reread(&bad, sizeof(bad), back)); }
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <golden tree file> <decode_plans.json>\n", argv[0]); return 2; }
    check_header();
    printf("header: ok\n");

    // the golden file (written by the reference): header, distance map, stream
    Stream gold;
    {
        FILE *f = fopen(argv[1], "rb");
        REQUIRE(f);
        Header h;
        REQUIRE(read_header(f, h));
        REQUIRE(h.X == 16 && h.Y == 16 && h.Z == 16 && h.origDepth == 12 && h.maxDepth == 12 + VR_CHAIN_LEVELS && h.rootMax[0] == 16);
        gold.D = h.origDepth;
        memset(gold.dmap, 0, sizeof(gold.dmap));
        REQUIRE(fread(gold.dmap, 1, (size_t)h.maxDepth + 1, f) == (size_t)h.maxDepth + 1);
        std::vector<uint8_t> bytes((size_t)(h.numActive + 3) / 4);
        REQUIRE(fread(bytes.data(), 1, bytes.size(), f) == bytes.size());
        fclose(f);
        for (int64_t i = 0; i < h.numActive; ++i) gold.tok.push_back((uint8_t)((bytes[(size_t)i / 4] >> (2 * (i % 4))) & 3));
    }
    std::vector<Stream> streams(1, gold);
    for (int D : {6, 9, 12})
        for (uint32_t prune : {30u, 150u, 400u}) {
            Stream s;
            s.D = D;
            for (uint8_t &d : s.dmap) d = (uint8_t)rnd();
            do { s.tok.clear(); gen_subtree(s, 0, prune); } while (s.tok.size() < 2);     // (not just a pruned root)
            streams.push_back(s);
        }
    printf("walker: %zu streams\n", streams.size());
    for (const Stream &s : streams) { check_walker(s); check_malformed(s); }

    // the fixture: every integer after "plans"
    Fixture fx;
    {
        FILE *f = fopen(argv[2], "rb");
        REQUIRE(f);
        std::string text;
        char buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, got);
        fclose(f);
        const size_t at = text.find("\"plans\"");
        REQUIRE(at != std::string::npos);
        for (const char *p = text.c_str() + at + 7; *p;) {
            if ((*p >= '0' && *p <= '9') || *p == '-') { char *end; fx.v.push_back(strtoll(p, &end, 10)); p = end; }
            else ++p;
        }
        REQUIRE(fx.v.size() == 1331u * (3 + 17 + 32));
    }
    check_geometry(fx);
    printf("geometry and plans: 1331 extent triples ok\n");
    return 0;
}
