// host_plan.h -- the codec's host logic that needs no device: the split rule and what follows from it, the launch
// geometry of the tiled kernels (planned once per set, at vr_brickset_create), the walker of foreign streams and the
// file header; and the error-bounded selection of cuts, vr_lod_select_error (declared in vrhip.h, defined in
// host_plan.cpp: a rule on a host table).  Includes no HIP header: compiles with a plain C++17 compiler (tests/host_plan_main.cpp links it
// directly) and with hipcc.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <array>
#include <vector>

#if defined(__HIP__) || defined(__HIPCC__)
#define VR_HD __host__ __device__
#else
#define VR_HD
#endif

#define VR_MAX_DEPTH 40     // origTreeDepth + 7 must stay below this
#define VR_CHAIN_LEVELS 7   // maxAddLevels (R.cpp:22)
#define VR_IDX_DEAD 0xFFFFFFFFu

namespace vr {

// Split geometry of one brick (power-of-two extents).  Passed to kernels by value.
struct Geom {
    int32_t D;                  // origTreeDepth
    int32_t nb[3];              // log2 of X, Y, Z
    int32_t X, Y, Z;
    uint8_t axis[32];           // split axis at depth d (d < D)
    uint8_t bit[32];            // coordinate bit decided at depth d
    int64_t voxels;             // X*Y*Z
};

// rank (D bits, MSB = depth 0) -> voxel coordinates
VR_HD inline void rank_to_xyz(const Geom &g, uint32_t r, int &x, int &y, int &z)
{
    int c[3] = {0, 0, 0};
    for (int d = 0; d < g.D; ++d) {
        uint32_t b = (r >> (g.D - 1 - d)) & 1u;
        c[g.axis[d]] |= (int)(b << g.bit[d]);
    }
    x = c[0]; y = c[1]; z = c[2];
}

// decoder step (R.cpp:783-787): child scalar from parent scalar and the child's code
VR_HD inline int apply_code(int v, int code, int dist)
{
    if (code == 1) { v += dist; return v > 255 ? 255 : v; }
    if (code == 2) { v -= dist; return v < 0 ? 0 : v; }
    return v;
}

// The breadth-first 2-bit codes are packed four per byte in heap order (TwoBitArray packing:
// element i in byte i/4, bits 2*(i&3)).
VR_HD inline int cget(const uint8_t *C, int64_t i) { return (C[i >> 2] >> ((int)(i & 3) * 2)) & 3; }

// ---- the split rule (buildRecursive, R.cpp:151-159) and what follows from it ----
void make_geom(Geom &g, const int64_t dims[3]);
// [c][k]: splits on axis k among depths 0 .. c-1, for c = 0 .. depths
std::vector<std::array<int, 3>> split_counts(const int64_t dims[3], int depths);
// local rank inside a depth-(D-K) subtree -> packed voxel offset (dx | dy<<10 | dz<<20)
std::vector<uint32_t> make_lut(const Geom &g, int K);
// rank bits of every x, y, z coordinate: rank(x,y,z) = spread[x] | spread[X+y] | spread[X+Y+z].  Kernels never walk
// Geom::axis/bit (a dependent chain of loads from the kernel-argument segment): a coordinate's contribution to the
// Morton rank comes from this table
std::vector<uint32_t> make_spread(const Geom &g);

// ---- launch geometry, fixed when a set is created (the pointers and the cut are added per call) ----
constexpr int VR_RG_REGX = 128;     // k_decode_region: x extent of a region (kd_decode.hip RG_REGX), 2^7

struct TilePlan {               // k_decode_tile / fine / quad: the geometry fields of TileArgs (kd_decode.hip), as named there
    bool ok;
    int jx, jy, jz, tilesX, tilesY, tilesZ, ltx, lty;
    uint8_t kqBit[8];
};
struct RegionPlan {             // k_decode_region: the geometry fields of RegionArgs (kd_decode.hip), as named there
    bool ok;
    int X, Y, lrx, lry, jx, nreg;
    int64_t voxels;
    uint32_t lanePos, parkP[4], parkS, gAddr[4], gByte, gOut[8], xRead[2], blkX, blkY, blkZ;
};
struct Pyr12Plan {              // k_pyramid12: the geometry fields of Pyr12Geom (kd_encode.hip), as named there
    bool use12;                 // every thread loads a 16-byte x-run of the caller's voxels (vrhip.h "alignment of caller buffers")
    int ax, ay, az, swz, nbx, nby, lnbx, lnby;
    uint16_t sx[16];
    bool lines;                 // k_pyramid12_lines applies: 16-voxel-wide boxes (ax == 4), eight of them per 128-byte line (X >= 128)
};
void make_plans(const Geom &g, int K, bool generalGeom, bool idx64, int64_t treeCap, TilePlan &tile, RegionPlan &region,
                Pyr12Plan &pyr12);

// ---- foreign streams (host): one preorder walk over the 2-bit tokens, grammar checked ----
// Per tree token node(depth, path, pos, tok, val): val is the node's decoded scalar, refined down to depth `cut` only; then
// pruned(depth, path, val) if the token ends the subtree (a 3), and chain(path) per token of the grown branch below
// leaf `path`.  Returns 0, or -1 / -2 (the stream ends inside the tree / inside a grown branch), -3 (tokens left
// over).  Reads tokens [0, numActive) only.
template <class Node, class Pruned, class Chain>
int walk_stream(int D, const uint8_t *tree, int64_t numActive, const uint8_t *dmap, int cut, Node node, Pruned pruned,
                Chain chain)
{
    int v[VR_MAX_DEPTH];
    int64_t pos = 0;
    int j = 0;
    uint32_t path = 0;
    while (true) {
        if (pos >= numActive) return -1;
        const int tok = cget(tree, pos);
        const int val = j == 0 ? dmap[0] : (j <= cut ? apply_code(v[j - 1], tok, dmap[j]) : v[j - 1]);
        v[j] = val;
        node(j, path, pos++, tok, val);
        bool terminal = tok == 3;
        if (terminal) pruned(j, path, val);
        else if (j == D) {
            for (int c = 1; c <= VR_CHAIN_LEVELS; ++c) {
                if (pos >= numActive) return -2;
                chain(path);
                if (cget(tree, pos++) == 3) break;
            }
            terminal = true;
        }
        if (terminal) {
            while (j > 0 && (path & 1u)) { path >>= 1; --j; }
            if (j == 0) break;
            path |= 1u;
        } else { ++j; path <<= 1; }
    }
    return pos == numActive ? 0 : -3;
}

// progressive cut above the index level: scalar of every depth-Ds subtree's ancestor at depth `cut` (< Ds)
int cut_values_from_stream(int D, int Ds, int K, int64_t nIdx, const uint8_t *tree, int64_t numActive,
                           const uint8_t *dmap, int cut, std::vector<uint8_t> &vals);
// the side-car index from the bytes alone: token offset and scalar of every depth-Ds root; with K == 6 also the
// tokens owned by each 4-leaf subtree (fine) and the scalar of every depth-(D-3) node (val3)
int build_index_from_stream(int D, int Ds, int K, int64_t nIdx, const uint8_t *tree, int64_t numActive,
                            const uint8_t *dmap, std::vector<uint32_t> &offs, std::vector<uint8_t> &vals,
                            std::vector<uint8_t> &fine, std::vector<uint8_t> &val3);

// ---- the file header of VolumeKdtree::save (R.cpp:535-544) and MidRangeTree::save (M.cpp:753-785) ----
struct Header { int64_t rootMin[3], rootMax[3]; int32_t maxDepth, origDepth; int64_t X, Y, Z, numActive; };
constexpr int VR_HEADER_BYTES = 88;
static_assert(sizeof(Header) == VR_HEADER_BYTES, "the header is written as it lies in memory");
// false: short read, maxDepth outside [VR_CHAIN_LEVELS, VR_MAX_DEPTH) or numActive <= 0
bool read_header(FILE *f, Header &h);
bool write_header(FILE *f, const Header &h);

} // namespace vr
