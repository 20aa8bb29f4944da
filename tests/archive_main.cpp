// archive_main.cpp -- stand-alone checks of the block table, the per-block index walker and the brick-set archive of
// volumerenderer_amd/csrc/host_plan.{h,cpp} (tests/test_archive_cpu.py builds it with the address and undefined-
// behaviour sanitizers and runs it).  No device, no Python.  index_block_walk and block_gap_walk are the very functions
// k_index_from_stream (kd_index.hip) runs, one lane per block; install() below is that kernel's lane loop written
// serially, over buffers sized exactly, so that a read or write outside them is a sanitizer report.
//   usage: archive_main <case file> <scratch directory>
// The case file (little-endian), written by the Python side from tests/refstream.py: int64 count, then per case
//   int64 X, Y, Z, D, numActive, treeBytes, nBlk, nIdx, stdChain; uint8 dmap[D + 8]; uint8 tree[treeBytes];
//   uint32 blockOff[nBlk]; uint8 topVal[2 nBlk]; uint8 idxTop[2 nIdx]      (the three expected, derived in NumPy)
#include "../volumerenderer_amd/csrc/host_plan.h"
#include "../include/vrhip.h"
#include <stdlib.h>
#include <string.h>
#include <string>

using namespace vr;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_ctx.c_str()); exit(1); } } while (0)
static std::string g_ctx;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;      // fixed seed: every run checks the same cases
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

struct Case {
    int64_t dims[3], D, numActive, treeBytes, nBlk, nIdx, stdChain;
    std::vector<uint8_t> dmap, tree, topVal, idxTop;
    std::vector<uint32_t> blockOff;
    int K() const { return D < 6 ? (int)D : 6; }
    int Ds() const { return (int)D - K(); }
    bool wantFine() const { return K() == 6 && D >= 6; }
};

template <class T> static void rd(FILE *f, T *p, size_t n) { REQUIRE(fread(p, sizeof(T), n, f) == n); }

static Case read_case(FILE *f)
{
    Case c;
    int64_t h[9];
    rd(f, h, 9);
    c.dims[0] = h[0]; c.dims[1] = h[1]; c.dims[2] = h[2]; c.D = h[3]; c.numActive = h[4]; c.treeBytes = h[5]; c.nBlk = h[6]; c.nIdx = h[7]; c.stdChain = h[8];
    c.dmap.resize((size_t)c.D + 8); c.tree.resize((size_t)c.treeBytes); c.blockOff.resize((size_t)c.nBlk);
    c.topVal.resize((size_t)c.nBlk * 2); c.idxTop.resize((size_t)c.nIdx * 2);
    rd(f, c.dmap.data(), c.dmap.size()); rd(f, c.tree.data(), c.tree.size()); rd(f, c.blockOff.data(), c.blockOff.size());
    rd(f, c.topVal.data(), c.topVal.size()); rd(f, c.idxTop.data(), c.idxTop.size());
    return c;
}

// a stream as the words the walker reads: exactly the words that hold its tokens, not one more
static std::vector<uint32_t> words_of(const std::vector<uint8_t> &tree, int64_t numActive)
{
    std::vector<uint32_t> w((size_t)((numActive + 15) / 16), 0u);
    const size_t n = std::min(tree.size(), w.size() * 4);
    if (n) memcpy(w.data(), tree.data(), n);
    return w;
}

struct Index {
    std::vector<uint32_t> off;
    std::vector<uint8_t> val, fine, val3, top;
    Index(const Case &c, bool fineToo)
        : off((size_t)c.nIdx, VR_IDX_DEAD), val((size_t)c.nIdx, 0), fine(fineToo ? (size_t)c.nIdx * 16 : 0, 0),
          val3(fineToo ? (size_t)c.nIdx * 8 : 0, 0), top((size_t)c.nIdx * 2, 0) {}
    BlockIndexOut out() { return BlockIndexOut{off.data(), val.data(), fine.empty() ? nullptr : fine.data(), val3.empty() ? nullptr : val3.data(), top.data()}; }
};

// vr_brickset_set_trees as far as it needs no device: the host's check of the table, then what the kernel's lanes do
static int install(const Case &c, const std::vector<uint32_t> &W, int64_t numActive, const std::vector<uint32_t> &tab,
                   const std::vector<uint8_t> &topVal, bool fineToo, Index &ix)
{
    if (!block_table_ok((int)c.D, numActive, tab.data())) return VR_ERR_FORMAT;
    const int Dc = block_depth((int)c.D);
    memcpy(ix.top.data(), topVal.data(), topVal.size());
    bool bad = false;
    uint8_t stack[VR_BLOCK_LEVELS + 1];
    const BlockIndexOut o = ix.out();
    for (int64_t p = 0; p < c.nBlk; ++p) {
        int status = 0;
        const uint32_t off = tab[(size_t)p];
        if (off != VR_IDX_DEAD && off >= (uint32_t)numActive) status = -4;
        else {
            uint32_t end = 0;
            if (p == 0) status = block_gap_walk(W.data(), (uint32_t)numActive, Dc, tab.data(), -1, 0u);
            const int v0 = ix.top[((size_t)1 << Dc) + (size_t)p];
            const int ws = index_block_walk(W.data(), (uint32_t)numActive, c.dmap.data(), (int)c.D, c.K(), (uint32_t)p, off, v0, o, stack, 1, &end);
            REQUIRE(end <= (uint32_t)numActive);
            if (status == 0) status = ws;
            if (status == 0 && off != VR_IDX_DEAD) status = block_gap_walk(W.data(), (uint32_t)numActive, Dc, tab.data(), p, end);
        }
        bad = bad || status != 0;
    }
    return bad ? VR_ERR_FORMAT : VR_OK;
}

// the walker of one block writes its own entries and no others
static void check_block_writes_stay_home(const Case &c, const std::vector<uint32_t> &W, int64_t numActive, const std::vector<uint32_t> &tab,
                                         const std::vector<uint8_t> &topVal)
{
    const int Dc = block_depth((int)c.D), Ds = c.Ds();
    const size_t per = (size_t)(c.nIdx / c.nBlk);
    for (int64_t p = 0; p < c.nBlk; ++p) {
        const uint32_t off = tab[(size_t)p];
        if (off != VR_IDX_DEAD && off >= (uint32_t)numActive) continue;
        Index ix(c, c.wantFine());
        std::fill(ix.top.begin(), ix.top.end(), (uint8_t)0xEE);
        std::fill(ix.val.begin(), ix.val.end(), (uint8_t)0xEE);
        std::fill(ix.val3.begin(), ix.val3.end(), (uint8_t)0xEE);
        std::fill(ix.fine.begin(), ix.fine.end(), (uint8_t)0xEE);
        std::fill(ix.off.begin(), ix.off.end(), 0xEEEEEEEEu);
        uint8_t stack[VR_BLOCK_LEVELS + 1];
        uint32_t end = 0;
        index_block_walk(W.data(), (uint32_t)numActive, c.dmap.data(), (int)c.D, c.K(), (uint32_t)p, off, topVal[((size_t)1 << Dc) + (size_t)p],
                         ix.out(), stack, 1, &end);
        for (size_t i = 0; i < (size_t)c.nIdx; ++i) {
            if (i / per == (size_t)p) continue;
            REQUIRE(ix.off[i] == 0xEEEEEEEEu && ix.val[i] == 0xEE);
            for (size_t k = 0; k < 16 && !ix.fine.empty(); ++k) REQUIRE(ix.fine[i * 16 + k] == 0xEE);
            for (size_t k = 0; k < 8 && !ix.val3.empty(); ++k) REQUIRE(ix.val3[i * 8 + k] == 0xEE);
        }
        for (int L = 0; L <= Ds; ++L)
            for (size_t i = 0; i < ((size_t)1 << L); ++i) {
                const bool mine = L >= Dc && (i >> (L - Dc)) == (size_t)p;
                if (!mine) REQUIRE(ix.top[((size_t)1 << L) + i] == 0xEE);
            }
        REQUIRE(ix.top[0] == 0xEE);
    }
}

static std::vector<uint8_t> pack_tokens(const std::vector<uint8_t> &t)
{
    std::vector<uint8_t> b((t.size() + 3) / 4, 0);
    for (size_t i = 0; i < t.size(); ++i) b[i >> 2] |= (uint8_t)(t[i] << ((i & 3) * 2));
    return b;
}

static int g_malformedRefused = 0, g_scalarDecoded = 0, g_garbageRefused = 0;

static void check_case(const Case &c, const std::string &dir)
{
    const int D = (int)c.D, Dc = block_depth(D), Ds = c.Ds(), K = c.K();
    REQUIRE(c.nBlk == (int64_t)1 << Dc && c.nIdx == (int64_t)1 << Ds);
    // ---- 1. the table
    std::vector<uint32_t> tab((size_t)c.nBlk);
    std::vector<uint8_t> top((size_t)c.nBlk * 2);
    REQUIRE(block_table_from_stream(D, c.tree.data(), c.numActive, c.dmap.data(), tab.data(), top.data()) == 0);
    REQUIRE(tab == c.blockOff);
    REQUIRE(memcmp(top.data() + 1, c.topVal.data() + 1, top.size() - 1) == 0);
    REQUIRE(block_table_ok(D, c.numActive, tab.data()));
    {
        std::vector<uint32_t> t2((size_t)c.nBlk);
        std::vector<uint8_t> v2((size_t)c.nBlk * 2);
        REQUIRE(vr_stream_block_table(c.dims, c.tree.data(), c.treeBytes, c.numActive, c.dmap.data(), D + 8, t2.data(), v2.data()) == VR_OK);
        REQUIRE(t2 == tab && v2 == top);
        REQUIRE(vr_stream_block_table(c.dims, c.tree.data(), c.treeBytes, c.numActive, c.dmap.data(), D + 7, t2.data(), v2.data()) == VR_ERR_INVALID);
        REQUIRE(vr_stream_block_table(c.dims, c.tree.data(), c.treeBytes - 1, c.numActive, c.dmap.data(), D + 8, t2.data(), v2.data()) == VR_ERR_FORMAT);
    }
    // ---- 2. the walker, block by block, against the host's one-pass index
    std::vector<uint32_t> offs;
    std::vector<uint8_t> vals, fine, val3;
    REQUIRE(build_index_from_stream(D, Ds, K, c.nIdx, c.tree.data(), c.numActive, c.dmap.data(), offs, vals, fine, val3) == 0);
    const std::vector<uint32_t> W = words_of(c.tree, c.numActive);
    for (int fineToo = 0; fineToo <= (c.wantFine() ? 1 : 0); ++fineToo) {
        Index ix(c, fineToo != 0);
        REQUIRE(install(c, W, c.numActive, tab, top, fineToo != 0, ix) == VR_OK);
        REQUIRE(ix.off == offs && ix.val == vals);
        if (fineToo) REQUIRE(ix.fine == fine && ix.val3 == val3);
        REQUIRE(memcmp(ix.top.data() + 1, c.idxTop.data() + 1, ix.top.size() - 1) == 0);
    }
    check_block_writes_stay_home(c, W, c.numActive, tab, top);
    // ---- 3. the archive: three bricks, the middle one absent
    const std::string path = dir + "/set.vrbs";
    const ArchiveGeom g = {0, {c.dims[0], c.dims[1], c.dims[2]}, 3, D, D + VR_CHAIN_LEVELS};
    std::vector<ArchiveBrick> bricks(3);
    for (int b = 0; b < 3; b += 2) {
        bricks[(size_t)b].numActive = c.numActive; bricks[(size_t)b].dmap = c.dmap.data(); bricks[(size_t)b].tree = c.tree.data();
        bricks[(size_t)b].blockOff = tab; bricks[(size_t)b].topVal = top;
    }
    {
        FILE *f = fopen(path.c_str(), "wb");
        REQUIRE(f && archive_write(f, g, bricks));
        REQUIRE(fclose(f) == 0);
    }
    std::vector<uint32_t> blobW;
    int64_t bytes = 0;
    {
        FILE *f = fopen(path.c_str(), "rb");
        REQUIRE(f);
        fseek(f, 0, SEEK_END); bytes = ftell(f); fseek(f, 0, SEEK_SET);
        REQUIRE(bytes > 0 && bytes % 16 == 0);
        blobW.resize((size_t)bytes / 4);
        rd(f, blobW.data(), blobW.size());
        fclose(f);
    }
    uint8_t *blob = (uint8_t *)blobW.data();
    ArchiveGeom g2;
    std::vector<ArchiveEntry> dirE;
    REQUIRE(archive_parse(blob, bytes, g2, dirE) == 0);
    REQUIRE(g2.variant == 0 && g2.numBricks == 3 && g2.D == D && g2.maxDepth == D + 7 && g2.dims[0] == c.dims[0] && g2.dims[1] == c.dims[1] && g2.dims[2] == c.dims[2]);
    REQUIRE(dirE.size() == 3 && dirE[1].offset == 0);
    for (int b = 0; b < 3; b += 2) {
        const ArchiveEntry &e = dirE[(size_t)b];
        REQUIRE(e.offset % 16 == 0 && e.numActive == c.numActive && e.treeBytes == c.treeBytes);
        const ArchiveRecord r = archive_record(blob, g2, e);
        REQUIRE(memcmp(r.dmap, c.dmap.data(), (size_t)D + 8) == 0 && memcmp(r.topVal, top.data(), top.size()) == 0);
        REQUIRE(memcmp(r.blockOff, tab.data(), tab.size() * 4) == 0 && memcmp(r.tree, c.tree.data(), c.tree.size()) == 0);
        REQUIRE(((uintptr_t)r.topVal - (uintptr_t)blob) % 16 == 0 && ((uintptr_t)r.blockOff - (uintptr_t)blob) % 16 == 0 && ((uintptr_t)r.tree - (uintptr_t)blob) % 16 == 0);
    }
    // ---- 4. malformed archives: refused by the parse alone
    {
        const auto refused = [&](const std::vector<uint32_t> &w, int64_t n) {
            ArchiveGeom gg; std::vector<ArchiveEntry> dd;
            return archive_parse(w.data(), n, gg, dd) != 0;
        };
        std::vector<uint32_t> m = blobW;
        ((uint8_t *)m.data())[0] ^= 1;                                  // the magic
        REQUIRE(refused(m, bytes));
        m = blobW; ((uint8_t *)m.data())[8] = 2;                        // the version
        REQUIRE(refused(m, bytes));
        m = blobW; ((uint8_t *)m.data())[dirE[2].offset + 5] ^= 0x10;   // a record byte: the checksum
        REQUIRE(refused(m, bytes));
        m = blobW; ((uint8_t *)m.data())[bytes - 1] ^= 0x80;            // the last byte (stream or padding)
        REQUIRE(refused(m, bytes));
        m = blobW;                                                      // a directory entry past the end of the file
        { ArchiveEntry e = dirE[2]; e.offset = bytes - 16; memcpy((uint8_t *)m.data() + VR_ARCHIVE_HEADER_BYTES + 2 * VR_ARCHIVE_ENTRY_BYTES, &e, sizeof(e)); }
        REQUIRE(refused(m, bytes));
        m = blobW;
        { ArchiveEntry e = dirE[2]; e.offset = bytes + 16; memcpy((uint8_t *)m.data() + VR_ARCHIVE_HEADER_BYTES + 2 * VR_ARCHIVE_ENTRY_BYTES, &e, sizeof(e)); }
        REQUIRE(refused(m, bytes));
        REQUIRE(refused(blobW, bytes - 16));                            // a file cut short
        REQUIRE(refused(blobW, 48));
    }
    // ---- 4. malformed streams and tables: VR_ERR_FORMAT, no report from the sanitizers
    std::vector<uint8_t> tok((size_t)c.numActive);
    for (int64_t i = 0; i < c.numActive; ++i) tok[(size_t)i] = (uint8_t)cget(c.tree.data(), i);
    const auto refuses = [&](const std::vector<uint8_t> &t, const std::vector<uint32_t> &tb, const std::vector<uint8_t> &tv) {
        const std::vector<uint8_t> packed = pack_tokens(t);
        const std::vector<uint32_t> w = words_of(packed, (int64_t)t.size());
        Index ix(c, c.wantFine());
        const int rc = t.empty() ? VR_ERR_FORMAT : install(c, w, (int64_t)t.size(), tb, tv, c.wantFine(), ix);
        if (!t.empty()) check_block_writes_stay_home(c, w, (int64_t)t.size(), tb, tv);
        return rc;
    };
    for (int drop = 1; drop <= 3; ++drop) {             // cut short: in the tree or in a grown branch, as the stream has it
        if ((int64_t)tok.size() <= drop) continue;
        std::vector<uint8_t> t(tok.begin(), tok.end() - drop);
        REQUIRE(refuses(t, tab, top) == VR_ERR_FORMAT);
        std::vector<uint32_t> t2((size_t)c.nBlk); std::vector<uint8_t> v2((size_t)c.nBlk * 2);
        const std::vector<uint8_t> packed = pack_tokens(t);
        const int ws = block_table_from_stream(D, packed.data(), (int64_t)t.size(), c.dmap.data(), t2.data(), v2.data());
        REQUIRE(ws == -1 || ws == -2);
        ++g_malformedRefused;
    }
    for (int extra = 0; extra < 4; ++extra) {           // tokens left over
        std::vector<uint8_t> t = tok;
        t.push_back((uint8_t)extra);
        REQUIRE(refuses(t, tab, top) == VR_ERR_FORMAT);
        ++g_malformedRefused;
    }
    std::vector<size_t> live;
    for (size_t p = 0; p < tab.size(); ++p) if (tab[p] != VR_IDX_DEAD) live.push_back(p);
    if (!live.empty()) {
        std::vector<uint32_t> tb = tab;
        tb[live.back()] = (uint32_t)c.numActive;        // an offset at the end of the stream
        REQUIRE(refuses(tok, tb, top) == VR_ERR_FORMAT);
        tb[live.back()] = VR_IDX_DEAD - 1u;
        REQUIRE(refuses(tok, tb, top) == VR_ERR_FORMAT);
        for (size_t p : live)                           // off by one, either way, every live block in turn
            for (int d = -1; d <= 1; d += 2) {
                tb = tab;
                tb[p] += (uint32_t)d;
                REQUIRE(refuses(tok, tb, top) == VR_ERR_FORMAT);
                ++g_malformedRefused;
            }
        tb = tab; tb[live[rnd() % live.size()]] = VR_IDX_DEAD;      // a live block called dead
        REQUIRE(refuses(tok, tb, top) == VR_ERR_FORMAT);
    }
    if (live.size() >= 2) {                             // offsets that do not increase
        std::vector<uint32_t> tb = tab;
        std::swap(tb[live[0]], tb[live[1]]);
        REQUIRE(refuses(tok, tb, top) == VR_ERR_FORMAT);
        tb = tab; tb[live[1]] = tb[live[0]];
        REQUIRE(refuses(tok, tb, top) == VR_ERR_FORMAT);
        ++g_malformedRefused;
    }
    for (size_t p = 0; p < tab.size(); ++p)
        if (tab[p] == VR_IDX_DEAD) {                    // a dead block called live, somewhere the host's check lets it be
            std::vector<uint32_t> tb = tab;
            uint32_t lo = (uint32_t)Dc, hi = (uint32_t)c.numActive;
            for (size_t q = 0; q < p; ++q) if (tab[q] != VR_IDX_DEAD) lo = tab[q] + 1u;
            for (size_t q = tab.size(); q-- > p + 1;) if (tab[q] != VR_IDX_DEAD) hi = tab[q];
            if (lo >= hi || (p == 0 && (lo > (uint32_t)Dc))) break;
            tb[p] = p == 0 ? (uint32_t)Dc : lo + rnd() % (hi - lo);
            REQUIRE(block_table_ok(D, c.numActive, tb.data()));
            REQUIRE(refuses(tok, tb, top) == VR_ERR_FORMAT);
            ++g_malformedRefused;
            break;
        }
    {   // a wrong start scalar: not detected -- other values, the same offsets and counts
        std::vector<uint8_t> tv = top;
        tv[((size_t)1 << Dc) + (live.empty() ? 0 : live[rnd() % live.size()])] ^= 0x55;
        const std::vector<uint32_t> w = words_of(c.tree, c.numActive);
        Index ix(c, c.wantFine());
        REQUIRE(install(c, w, c.numActive, tab, tv, c.wantFine(), ix) == VR_OK);
        REQUIRE(ix.off == offs);
        if (c.wantFine()) REQUIRE(ix.fine == fine);
        ++g_scalarDecoded;
    }
    for (int round = 0; round < 6; ++round) {           // bytes that are no stream at all, with the good table
        std::vector<uint8_t> t = tok;
        if (round < 3) for (int k = 0; k < 1 + (int)(t.size() / 64); ++k) t[rnd() % t.size()] = (uint8_t)(rnd() & 3u);
        else for (auto &x : t) x = (uint8_t)(round == 3 ? rnd() & 3u : (round == 4 ? 0 : 3));
        const int rc = refuses(t, tab, top);
        REQUIRE(rc == VR_OK || rc == VR_ERR_FORMAT);
        if (rc == VR_ERR_FORMAT) ++g_garbageRefused;
        else {      // accepted: then it IS a stream of the grammar, and the index is the host's
            const std::vector<uint8_t> packed = pack_tokens(t);
            std::vector<uint32_t> o2; std::vector<uint8_t> a2, f2, b2;
            REQUIRE(build_index_from_stream(D, Ds, K, c.nIdx, packed.data(), (int64_t)t.size(), c.dmap.data(), o2, a2, f2, b2) == 0);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: archive_main <case file> <scratch directory>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    REQUIRE(f);
    int64_t count = 0;
    rd(f, &count, 1);
    for (int64_t i = 0; i < count; ++i) {
        const Case c = read_case(f);
        g_ctx = "case " + std::to_string(i) + ": " + std::to_string(c.dims[0]) + "x" + std::to_string(c.dims[1]) + "x" + std::to_string(c.dims[2]);
        check_case(c, argv[2]);
    }
    fclose(f);
    REQUIRE(fnv1a64((const uint8_t *)"a", 1) == 0xaf63dc4c8601ec8cull);       // the published test vector
    REQUIRE(g_malformedRefused > 0 && g_scalarDecoded == count);
    printf("archive unit: %lld cases ok (%d malformed inputs refused, %d of %lld garbage streams refused)\n", (long long)count,
           g_malformedRefused, g_garbageRefused, (long long)(6 * count));
    return 0;
}
