// host_select_main.cpp -- vr_lod_select_error (volumerenderer_amd/csrc/host_plan.cpp) on edge tables, as a stand-alone
// program: tests/test_error_table_cpu.py builds it with plain g++ under the address and undefined-behaviour sanitizers,
// links host_plan.cpp and nothing else, and runs it as a child process.  Tables are heap vectors of exactly the size
// the call may read, so a read past a row or a brick is caught.
#include "../include/vrhip.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static vr_brick_error entry(uint32_t max_abs, uint64_t sum_sq)
{
    vr_brick_error e;
    e.sum_abs = sum_sq; e.sum_sq = sum_sq; e.max_abs = max_abs; e.num_diff = max_abs ? 1u : 0u;
    return e;
}

static std::vector<int32_t> select(const std::vector<vr_brick_error> &t, int32_t B, int32_t lo, int32_t hi, int64_t V,
                                   const std::vector<int32_t> *in, int32_t bound, double msb, vr_status want = VR_OK)
{
    std::vector<int32_t> out((size_t)B, 12345);
    const vr_status s = vr_lod_select_error(t.data(), B, lo, hi, V, in ? in->data() : nullptr, bound, msb, out.data());
    CHECK(s == want);
    return out;
}

int main()
{
    static_assert(sizeof(vr_brick_error) == 24, "vr_brick_error is 24 bytes");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    {   // one cut, one brick
        const std::vector<vr_brick_error> t = {entry(0, 0)};
        CHECK(select(t, 1, 5, 5, 64, nullptr, 0, -1.0)[0] == 5);
        const std::vector<vr_brick_error> u = {entry(3, 9)};
        CHECK(select(u, 1, 5, 5, 64, nullptr, 0, -1.0)[0] == 5);          // none qualifies: h
        CHECK(select(u, 1, 5, 5, 64, nullptr, 3, -1.0)[0] == 5);
        const std::vector<int32_t> below = {2}, above = {40}, culled = {-1};
        CHECK(select(t, 1, 5, 5, 64, &below, 0, -1.0)[0] == 2);           // h < cut_lo: no candidate
        CHECK(select(t, 1, 5, 5, 64, &above, 0, -1.0)[0] == 5);           // candidates end at cut_hi
        CHECK(select(u, 1, 5, 5, 64, &above, 0, -1.0)[0] == 40);          // ... and h comes back as it is
        CHECK(select(t, 1, 5, 5, 64, &culled, 0, -1.0)[0] == -1);
    }
    {   // all -1: the table is never the answer
        const int B = 7, rows = 3;
        std::vector<vr_brick_error> t((size_t)(B * rows), entry(0, 0));
        const std::vector<int32_t> in((size_t)B, -1);
        const std::vector<int32_t> out = select(t, B, 0, rows - 1, 4096, &in, 0, 0.0);
        for (int b = 0; b < B; ++b) CHECK(out[(size_t)b] == -1);
    }
    {   // errors that do not fall with the cut; the bounds one at a time; the smallest qualifying cut wins
        const int B = 3, lo = 2, hi = 6;          // rows: cuts 2 .. 6
        std::vector<vr_brick_error> t((size_t)(B * (hi - lo + 1)));
        const uint32_t mx[5][3] = {{9, 0, 200}, {4, 7, 100}, {6, 0, 4}, {0, 1, 9}, {2, 0, 0}};
        const uint64_t sq[5][3] = {{900, 0, 70000}, {30, 640, 641}, {500, 0, 16}, {0, 1, 639}, {4, 0, 0}};
        for (int r = 0; r < 5; ++r) for (int b = 0; b < B; ++b) t[(size_t)(r * B + b)] = entry(mx[r][b], sq[r][b]);
        std::vector<int32_t> out = select(t, B, lo, hi, 64, nullptr, 0, -1.0);
        CHECK(out[0] == 5 && out[1] == 2 && out[2] == 6);
        out = select(t, B, lo, hi, 64, nullptr, 4, -1.0);
        CHECK(out[0] == 3 && out[1] == 2 && out[2] == 4);
        out = select(t, B, lo, hi, 64, nullptr, 255, 10.0);              // the mean-square bound alone: sum_sq <= 640
        CHECK(out[0] == 3 && out[1] == 2 && out[2] == 4);
        out = select(t, B, lo, hi, 64, nullptr, 255, 0.0);               // -0.0 and 0.0 are bounds, not "off"
        CHECK(out[0] == 5 && out[1] == 2 && out[2] == 6);
        out = select(t, B, lo, hi, 64, nullptr, 255, -0.0);
        CHECK(out[0] == 5 && out[1] == 2 && out[2] == 6);
        out = select(t, B, lo, hi, 64, nullptr, 255, inf);
        CHECK(out[0] == 2 && out[1] == 2 && out[2] == 2);
        const std::vector<int32_t> in = {4, -1, 3};
        out = select(t, B, lo, hi, 64, &in, 0, -1.0);
        CHECK(out[0] == 4 && out[1] == -1 && out[2] == 3);
        // 0.1 * 3 is 0.30000000000000004 in double: a sum of squares of 0 passes, 1 does not
        const std::vector<vr_brick_error> w = {entry(1, 1), entry(0, 0)};
        CHECK(select(w, 1, 0, 1, 3, nullptr, 255, 0.1)[0] == 1);
        // 2^32 - 1 voxels, each off by 255: the largest entry there is, and it meets its own mean exactly
        const std::vector<vr_brick_error> big = {entry(255, 65025ull * 0xFFFFFFFFull), entry(0, 0)};
        CHECK(select(big, 1, 0, 1, 0xFFFFFFFFll, nullptr, 255, 65025.0)[0] == 0);
        CHECK(select(big, 1, 0, 1, 0xFFFFFFFFll, nullptr, 255, 65024.0)[0] == 1);
    }
    {   // refused, and cuts_out untouched
        const std::vector<vr_brick_error> t = {entry(0, 0), entry(0, 0)};
        std::vector<int32_t> out(2, 777);
        CHECK(vr_lod_select_error(nullptr, 2, 0, 0, 64, nullptr, 0, -1.0, out.data()) == VR_ERR_INVALID);
        CHECK(vr_lod_select_error(t.data(), 2, 0, 0, 64, nullptr, 0, -1.0, nullptr) == VR_ERR_INVALID);
        CHECK(vr_lod_select_error(t.data(), 0, 0, 0, 64, nullptr, 0, -1.0, out.data()) == VR_ERR_INVALID);
        CHECK(vr_lod_select_error(t.data(), 2, -1, 0, 64, nullptr, 0, -1.0, out.data()) == VR_ERR_INVALID);
        CHECK(vr_lod_select_error(t.data(), 2, 1, 0, 64, nullptr, 0, -1.0, out.data()) == VR_ERR_INVALID);
        CHECK(vr_lod_select_error(t.data(), 2, 0, 0, 0, nullptr, 0, -1.0, out.data()) == VR_ERR_INVALID);
        CHECK(vr_lod_select_error(t.data(), 2, 0, 0, 64, nullptr, -1, -1.0, out.data()) == VR_ERR_INVALID);
        CHECK(vr_lod_select_error(t.data(), 2, 0, 0, 64, nullptr, 0, nan, out.data()) == VR_ERR_INVALID);
        const std::vector<int32_t> bad = {0, -2};
        CHECK(vr_lod_select_error(t.data(), 2, 0, 0, 64, bad.data(), 0, -1.0, out.data()) == VR_ERR_INVALID);
        CHECK(out[0] == 777 && out[1] == 777);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("selection rule: edge tables ok\n");
    return 0;
}
