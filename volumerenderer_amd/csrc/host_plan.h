// host_plan.h -- the codec's host logic that needs no device: the split rule and what follows from it, the launch
// geometry of the tiled kernels (planned once per set, at vr_brickset_create), the debugging switches' one table, the
// plan of a build (BuildPlan: every kernel, grid and brick range of vr_brickset_build), the plan of a decode call (DecodePlan /
// LodPlan: the kernel, grids, class lists and buffers of the uniform and per-brick decodes), the walker of foreign streams and the
// file header, the block tables and per-block index walker of installed streams (shared with kd_index.hip's kernel) and the
// brick-set archive's parser and writer, the plan of an install (InstallPlan: the refusals, host passes and buffers of
// vr_brickset_set_tree / _set_trees); and the error-bounded selection of cuts, vr_lod_select_error (declared in vrhip.h, defined in
// host_plan.cpp: a rule on a host table).  Includes no HIP header: compiles with a plain C++17 compiler (tests/host_plan_main.cpp links it
// directly) and with hipcc.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <array>
#include <functional>
#include <vector>

#if defined(__HIP__) || defined(__HIPCC__)
#define VR_HD __host__ __device__
#else
#define VR_HD
#endif

#define VR_MAX_DEPTH 40     // origTreeDepth + 7 must stay below this
#define VR_CHAIN_LEVELS 7   // maxAddLevels (R.cpp:22)
#define VR_IDX_DEAD 0xFFFFFFFFu

struct vr_pool_entry;       // vrhip.h
struct vr_tree_desc;

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

// ---- the start-distance estimator's rounds (kd_encode.hip "running-mean start distance") ----
// A level of n > VR_EST_HEAD nodes is nseg = n / VR_EST_SEG segments; the head walk covers the first four.  Round r
// summarises the segments from where a brick's walk stands up to segEnd under nc candidate thresholds around the
// brick's current one, and the walk then carries the exact state to segEnd, or to where the threshold leaves the
// window.  nseg is the same for every brick of a level, so the plan is a host constant per level.  quads: the round may
// run the byte-quad kernel with sufficient bounds (and counts against the brick's budget of node-by-node segments);
// the last round never does: it finishes the level whatever happens.  sweeps: segments a workgroup of the summary kernel
// takes, in eights -- few where most bricks take part, many in a round that picks up the few bricks that left an earlier one
// (its other workgroups only return).
constexpr int VR_EST_SEG = 1024, VR_EST_HEAD = 4096, VR_EST_CAND = 8, VR_EST_MAX_ROUNDS = 8;
struct EstRound { uint32_t segEnd; int32_t nc; bool quads; int32_t sweeps; };
struct EstPlan { int32_t rounds; EstRound r[VR_EST_MAX_ROUNDS]; };
// oldSchedule: every round over the whole level, 4-wide quads, 4-wide exact, then 8-wide exact ones
EstPlan est_round_plan(uint32_t nseg, bool oldSchedule);
// first threshold of a window of nc candidates around threshold T; `up`: the running mean S / (2C + 1) sits in the
// upper half of [T, T + 1), which orients a window that has no room for both neighbours
VR_HD inline int est_window_base(long long T, int up, int nc)
{
    long long b = T - (nc >= 8 ? 2 : (nc >= 3 ? 1 : (nc == 2 && !up ? 1 : 0)));
    if (b < 0) b = 0;
    if (b > 256 - nc) b = 256 - nc;
    return (int)b;
}

// ---- debugging switches ----
// Each runs one kernel in place of another on the same data, for the tests to compare.  ONE table (VR_SWITCHES) names
// them: vr_brickset_set_switch looks its argument up there, and vr_brickset_create reads VRHIP_<NAME in capitals> of
// the same rows from the environment, ONCE -- never in a launch path: the kernels a handle uses do not change behind
// the caller's back.  A switch is a member here and a row there; vrhip.h documents the names (tests/test_build_plan.py
// compares its list with the table).
constexpr int EST_QUAD_BUDGET = 8;  // per brick and level, over its quad rounds (once round 0's: EST_R0_BUDGET).  DESIGN.md 3.2: 8, 16 and 32 measured, 8 kept
struct Switches {
    bool decodeWalk = false;     // decode_walk: k_decode_tile (no per-4-leaf counts)
    bool decodeFineV1 = false;   // decode_fine_v1: round 1's k_decode_fine
    bool decodeQuad = false;     // decode_quad: round 2's k_decode_quad instead of k_decode_region
    bool noSkipBlocks = false;   // no_skip_blocks
    bool noUniformBlocks = false; // no_uniform_blocks: constant 4096-leaf blocks go through k_prune_emit12, not k_prune_emit12_const
    bool estExactBounds = false; // est_exact_bounds: the estimator's quad rounds run the exact k_est_summ<false>, with no fallback budget
    bool estOldSchedule = false; // est_old_schedule: every estimator round over the whole level, 4-wide quads first (est_round_plan)
    int estBudget = EST_QUAD_BUDGET; // VRHIP_EST_BUDGET=<n> only: node-by-node segments a brick may walk in a level's quad rounds (measurement aid)
    bool pyramidBoxes = false;   // pyramid_boxes: k_pyramid12 (one box per workgroup) where k_pyramid12_lines applies
    bool indexPerBlock = false;  // index_per_block: k_index12_block (a wave per 4096-leaf block) + k_const_finish over every index entry, not k_index12
    bool noUniformDecode = false; // no_uniform_decode: k_decode_region ignores BrickSet::boxUniform (every live box is parsed).  Read per call
};
struct SwitchRow { const char *name; bool Switches::*member; };
extern const SwitchRow VR_SWITCHES[];
extern const int VR_NUM_SWITCHES;
bool Switches::*find_switch(const char *name);      // nullptr: no row of that name
void switch_env_name(const char *name, char *out, size_t cap);   // "VRHIP_" + the name in capitals
Switches switches_from_env();

// ---- the build (kd_encode.hip encode_launch / compress_stream execute it; they decide nothing) ----
// Every decision of a build from plain inputs: which kernels, on which grids, over which brick ranges.  Contract with
// the allocator (capi.hip): blockFlag exists exactly when fused, blockFlagR when fused and MidRange; fineIdx, idxVal3 and
// boxUniform exist when fused; brickOff, compactOverflow and treeCompact when compact -- all before the first launch.
constexpr int FILL_ITERS = 8;                // chunks of 4096 nodes per workgroup of k_fill16 (large levels)
constexpr int FILL_NODES_PER_BLOCK = 1024;   // nodes per workgroup of k_fill (levels below 4096 nodes)
constexpr int VR_PEC_BOXES = 16, VR_IDX_BLOCKS = 32, VR_EMIT_RANKS = 256;    // kd_encode.hip PEC_BOXES, IDX_BLOCKS, EMIT_RANKS_PER_BLOCK
constexpr int VR_PYR_MAX_ROUNDS = 4, VR_MAX_PARTS = 4;

inline bool build_fused(int D) { return D >= 12; }     // BuildPlan::fused: also sizes a set's stream slots (vr_brickset_create)
struct BuildInputs {
    int32_t D, B, variant, tolerance, maxEpochs;
    bool use12, lines;          // Pyr12Plan
    bool generalGeom;
    Switches sw;
    int32_t levelLoopStreams;
    bool compactOnBuild;
    int32_t sideStreams;        // internal streams the handle has (at least build_side_streams() were asked for)
};
// internal streams a build would use beside the caller's: one for a MidRangeTree's half-range stream, one per further
// brick range of a VolumeKdtree
int build_side_streams(int variant, int B, int levelLoopStreams);

struct PyrRound { int32_t dLeaf, L; uint32_t blocks; };      // k_pyramid: L <= 10 levels from depth dLeaf up
enum IndexKernel { VR_INDEX12, VR_INDEX12_BLOCK, VR_EMIT_WRITE };
struct BuildPlan {
    int32_t D, B, maxEpochs;
    bool midRange, guarded;     // guarded: GUARDED and MIDRANGE both carry the R.cpp:333/:340 guard
    bool fused;                 // k_prune_emit12: prune + block-local emit in one kernel, 4096-leaf blocks
    bool leafless;              // the level loop keeps nothing of the leaf level (sizes the encoder's arrays)
    bool skipBlocks;            // kd_encode.hip SkipBlocks
    bool constClosedForm;       // constant bricks take k_const_finish's closed form
    bool zeroFill;              // no epoch runs: codes and reconstructions are zero-filled
    int64_t boxes;              // 4096-leaf boxes per brick, 2^max(D-12, 0): blockFlag, boxUniform, SkipBlocks::nBlk
    // pyramid: the bottom twelve levels by one of the k_pyramid12 kernels, the rest in rounds of k_pyramid; round 0
    // reads voxels (exactly when !pyr12), through srcIdx when pyrSrcIdx
    bool pyr12, pyr12Lines, pyrSrcIdx;
    uint32_t pyr12Grid;
    int32_t pyrRounds;
    PyrRound pyr[VR_PYR_MAX_ROUNDS];
    int64_t rootStride;         // bytes per brick of a carry array (mmMin / mmMax): 2^max(D-10, 0)
    // level loop: brick range i is [range[i], range[i+1]); range 0 on the caller's stream, range i on side stream i-1
    int32_t parts, range[VR_MAX_PARTS + 1];
    bool forkRange;             // the half-range stream's level loop on side stream 0
    bool estOldSchedule, estExactBounds;
    int32_t estBudget;
    // prune
    bool uniformBlocks;         // k_prune_emit12_const in front
    uint32_t uniformGrid, pruneGrid;     // pruneGrid: k_prune_emit12<RANGE, leafless> when fused, k_prune_leaf otherwise
    int32_t pruneFrom;          // k_prune_level from this depth up to 0
    // convert
    int32_t emitLeaves;         // leaves per emit block
    int64_t nblk;               // emit blocks per brick
    IndexKernel index;
    uint32_t indexGrid;
    uint32_t constFinishGrid, constFinishThreads;
    int64_t constFinishIdx;     // index entries per brick k_const_finish writes (0: k_index12 wrote them)
    int64_t statRecords;        // k_emit_stats: records per brick
    bool gapped, compact;
};
BuildPlan make_build_plan(const BuildInputs &in);

// one level (n = 2^d nodes) of the level loop
struct EstLaunch { uint32_t gx; bool quads; int32_t budget; };      // k_est_summ<quads> on gx workgroups per brick
// eight segments per workgroup and sweep (two per wave).  A quad round makes R.sweeps sweeps over the segments a brick
// can still have in front of it; the exact rounds behind them run on a small grid.  Quad rounds: byte-packed quads with
// sufficient bounds, and the level's budget of node-by-node segments per brick (exactBounds: the exact kernel, no
// budget, -1); the rounds behind them: exact records
EstLaunch est_launch(const EstRound &R, bool exactBounds, int32_t budget);
struct BuildLevel {
    bool constLeaves;           // k_fill_const_leaves in front: the skip bits are final (level D-2 has ended)
    EstPlan est;                // rounds == 0: k_est_head covers the level
    EstLaunch estL[VR_EST_MAX_ROUNDS];
    bool fill16;                // k_fill16<!sumsOnly> with iters chunks per workgroup; else k_fill
    bool sumsOnly;              // the leaf level of a leafless build: errors only
    int32_t iters;
    uint32_t fillGrid;
};
BuildLevel build_level(const BuildPlan &p, int d);

// ---- a decode (kd_decode.hip decode_launch / decode_lod_launch execute it; they decide nothing) ----
// Every decision of a decode call from plain inputs, gathered from the set when the call arrives: which kernel, on
// which grid, with which companions, where the cut values come from and which buffers the launches touch.  Contract with
// the allocator (capi.hip ensure_decode_buffers / ensure_lod_slot): everything in `needs` exists, and the quad tables are
// written, before the first launch.
constexpr int VR_DEC_WAVES = 4, VR_FD_WAVES = 4, VR_FD_TABLE_WORDS = 1024 + 64 + 4;       // kd_decode.hip DEC_WAVES, FD_*, QD_*, RG_*
constexpr int VR_QD_WAVES = 16, VR_QD_TPW = 16, VR_QD_CHAIN_ENTRIES = 16384, VR_RG_PER = 16, VR_RG_WAVES = 8;
constexpr int VR_RG_MIN_WGS = 2048;         // k_decode_region: at least this many workgroups where the regions allow it
constexpr int VR_STAGE_BRICKS = 32;         // vrhip.h VR_POOL_STAGE_BRICKS

// the kernels, in the order a per-brick decode launches its classes
enum class DecodeKernel { REGION, QUAD, FINE, TILE, GENERAL, LANE };
constexpr int DECODE_KERNELS = (int)DecodeKernel::LANE + 1;
// scalars above depth Ds: none needed; k_cut_values from the encoder's codes; or written before the launch by the
// caller (a set of installed streams: capi.hip foreign_cut_values)
enum class CutSource { NONE, CODES, CALLER };

struct DecodeInputs {
    int32_t D, Ds, B, nb0;      // nb0: log2 X
    int64_t nIdx, voxels, leafStride, nEmitBlk;
    bool generalGeom, idx64;
    bool tileOk; int32_t tiles;         // TilePlan: ok, tilesX * tilesY * tilesZ
    bool regionOk; int32_t nreg;        // RegionPlan
    bool fineAll;               // every brick has the per-4-leaf side-car (fineIdx && fineAll)
    bool idxVal3, foreign, rangeStream;
    bool decodeWalk, decodeFineV1, decodeQuad, noUniformDecode;     // Switches, read per call
};
struct DecodeNeeds { bool rankVals, decTables, chainTab, idxValCut; };
// one launch of a decode kernel on grid (gx, rows) x threads; a per-brick decode: over image[first .. first + rows)
struct DecodeLaunch {
    DecodeKernel kernel;
    int32_t rows, cut;          // cut: the call's, or one of the class's (the kernels read each row's own)
    uint32_t gx, threads;
    uint32_t gatherGx;          // GENERAL: k_owner_gather on (gatherGx, rows) x 256 behind it
    bool fineTables;            // FINE: k_fine_tables on rows x 256 in front
    int32_t chainLevels;        // QUAD: the table of that many refining levels (a per-brick decode: 0, the kernel adds each row's)
    int32_t pass, first;        // per-brick decode: 0 = to the caller's buffer, p >= 1 = staged batch p - 1
    bool waitStage;             // the call's first staged launch: the staging buffer's previous reader comes first
    int32_t packRows, packFirst;    // the batch's last class: k_pool_pack over packRows descriptors from packFirst follows
};
struct DecodePlan {
    DecodeLaunch launch;
    bool rangeStream;
    CutSource cutValues;
    int32_t cutAll;             // k_cut_values' depth: min(cut, Ds)
    bool idxValFromCut;         // the range stream's index scalars are the cut values
    bool uni;                   // k_decode_region gets the uniform-box hint
    int64_t nBase;              // GENERAL with 64-bit offsets: block-relative index entries, this many bases per brick
    bool storesVectors;         // 16-byte stores to the caller's buffer (vrhip.h "alignment of caller buffers")
    DecodeNeeds needs;
};
DecodePlan make_decode_plan(const DecodeInputs &in, int cut);

// vr_brickset_decode_lod / _lod_pool.  cuts: per brick, -1 = skipped.  topIndexed: per brick of a foreign set, its cut
// values come from idxTop (null: of none).  off / shift: pool_layout's (null: no pool); tableCells: the pool table to
// upload (0: none).  With a pool the full-resolution bricks go straight to their slots (pass 0), the coarse ones
// VR_STAGE_BRICKS at a time, in index order, to the staging buffer, each batch followed by k_pool_pack.
struct LodPlan {
    std::vector<int32_t> image;     // cuts [0, B), the bricks cut above Ds (nTop from idxTop first), then the class lists
    int32_t nAbove, nTop, nRows;    // nRows: decoded bricks
    std::vector<DecodeLaunch> launches;
    std::vector<int64_t> offsets;   // pool: each list entry's output offset [0, nRows), from B on the pack descriptors
                                    // (slot offset, sx | sy << 8 | sz << 16), batch by batch; else empty
    uint32_t packGx;
    CutSource cutValues;
    bool uni, staged, storesVectors;
    int64_t nBase;
    bool nothing;                   // every brick skipped and no table: nothing to launch
    DecodeNeeds needs;              // of the slot (chainTab: the set's)
    int64_t tableCells;
};
LodPlan make_lod_plan(const DecodeInputs &in, const int32_t *cuts, const uint8_t *topIndexed, const int64_t *off,
                      const uint8_t *shift, int64_t tableCells);

// vr_lod_pool_layout's rule (vrhip.h); returns a vr_status.  off / shift: per brick (shift 3 bytes each), may be null;
// table: per grid cell, may be null.
int pool_layout(const int64_t bd[3], int32_t nb, const int64_t *ijk, const int64_t grid[3], const int32_t *cuts,
                int32_t origDepth, int32_t maxDepth, int64_t *off, uint8_t *shift, vr_pool_entry *table, int64_t *total);

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

// ---- block tables: the index of a stream rebuilt block by block (vrhip.h "compressed brick-set archives") ----
// A block is a depth-Dc node, Dc = max(D - 12, 0): a 4096-leaf box where D >= 12, the whole brick otherwise.  The table
// of a stream: blockOff[2^Dc], the token index of every block root's own token (VR_IDX_DEAD: an ancestor was pruned),
// and topVal[2^(Dc+1)], a 1-based heap over depths 0 .. Dc ((1 << j) + path; entry 0 unused) of decoded scalars, a
// pruned node's scalar standing for every node below it.  A walk from blockOff[p] that starts with the scalar
// topVal[(1 << Dc) + p] sees what walk_stream sees below that node.
#define VR_BLOCK_LEVELS 12
#define VR_TREE_TAIL 2048    // bytes zeroed past an installed stream's end: no decoder reads further
VR_HD inline int block_depth(int D) { return D > VR_BLOCK_LEVELS ? D - VR_BLOCK_LEVELS : 0; }

// one walk_stream pass; 0 or walk_stream's status
int block_table_from_stream(int D, const uint8_t *tree, int64_t numActive, const uint8_t *dmap, uint32_t *blockOff,
                            uint8_t *topVal);
// what the host can say about a table without the stream: every live offset below numActive, live offsets strictly
// increasing with the block number, block 0 (the path that is never a right child) at token Dc when it is live, the
// only block of a shallow brick at token 0
bool block_table_ok(int D, int64_t numActive, const uint32_t *blockOff);

// token `pos` of a stream read as aligned 32-bit words, sixteen tokens each (little-endian: cget's packing)
VR_HD inline int wget(const uint32_t *W, uint32_t pos) { return (int)((W[pos >> 4] >> ((pos & 15u) * 2u)) & 3u); }

// One brick's index arrays.  fine / val3 null: the brick gets none (K != 6, D < 6 or a map that fails
// std_chain_distances).  top: 2 * nIdx bytes, a heap like topVal over depths 0 .. Ds.
struct BlockIndexOut { uint32_t *off; uint8_t *val, *fine, *val3, *top; };

// The walker of one block: the index entries below block `blk`, byte for byte what build_index_from_stream gives them
// (the entries are at their defaults when it starts: offsets VR_IDX_DEAD, everything else 0), and the scalars of its
// nodes of depths Dc .. Ds in o.top.  off / v0: the block's table entries.  stack: one byte per level Dc .. D (at most
// VR_BLOCK_LEVELS + 1), level l at stack[l * stride].  No token at or past numActive is read, nothing outside the
// block's own entries is written, and every iteration consumes a token: no byte pattern reads or writes elsewhere or
// runs it forever.  Returns 0 and the token after the block's subtree in *end, or -1 / -2 (the stream ends inside the
// tree / inside a grown branch).
VR_HD inline int index_block_walk(const uint32_t *W, uint32_t numActive, const uint8_t *dmap, int D, int K, uint32_t blk,
                                  uint32_t off, int v0, const BlockIndexOut &o, uint8_t *stack, int stride, uint32_t *end)
{
    const int Dc = block_depth(D), Ds = D - K;
    const bool fine = o.fine != nullptr;
    // a node pruned at depth j stands for every node below it (fill_below's rule, and the heap's)
    const auto below = [&](int j, uint32_t path, int val) {
        for (int L = j + 1; L <= Ds; ++L)
            for (uint32_t i = path << (L - j), e = (path + 1u) << (L - j); i < e; ++i) o.top[(1u << L) + i] = (uint8_t)val;
        if (j < Ds) for (uint32_t i = path << (Ds - j), e = (path + 1u) << (Ds - j); i < e; ++i) o.val[i] = (uint8_t)val;
        if (fine && j < D - 3) for (uint32_t i = path << (D - 3 - j), e = (path + 1u) << (D - 3 - j); i < e; ++i) o.val3[i] = (uint8_t)val;
    };
    *end = 0;
    if (off == VR_IDX_DEAD) { o.top[(1u << Dc) + blk] = (uint8_t)v0; below(Dc, blk, v0); return 0; }
    // tokens of depth >= Ds belong to the 4-leaf subtree that holds their node's first leaf; in preorder those
    // subtrees never go back, so one count is open at a time
    uint32_t grp = 0;
    int cnt = 0, status = 0;
    const auto own = [&](uint32_t firstLeaf) {
        const uint32_t g = firstLeaf >> 2;
        if (cnt && g != grp) { o.fine[grp] = (uint8_t)cnt; cnt = 0; }
        grp = g; ++cnt;
    };
    uint32_t pos = off, path = blk;
    int j = Dc;
    while (true) {
        if (pos >= numActive) { status = -1; break; }
        const int tok = wget(W, pos);
        const int val = j == Dc ? v0 : apply_code(stack[(j - 1 - Dc) * stride], tok, dmap[j]);
        stack[(j - Dc) * stride] = (uint8_t)val;
        if (j <= Ds) o.top[(1u << j) + path] = (uint8_t)val;
        if (j == Ds) { o.off[path] = pos; o.val[path] = (uint8_t)val; }
        if (fine && j == D - 3) o.val3[path] = (uint8_t)val;
        if (fine && j >= Ds) own(path << (D - j));
        ++pos;
        bool terminal = tok == 3;
        if (terminal) below(j, path, val);
        else if (j == D) {
            for (int c = 1; c <= VR_CHAIN_LEVELS; ++c) {
                if (pos >= numActive) { status = -2; break; }
                if (fine) own(path);
                if (wget(W, pos++) == 3) break;
            }
            if (status) break;
            terminal = true;
        }
        if (terminal) {
            while (j > Dc && (path & 1u)) { path >>= 1; --j; }
            if (j == Dc) break;
            path |= 1u;
        } else { ++j; path <<= 1; }
    }
    if (cnt) o.fine[grp] = (uint8_t)cnt;
    *end = pos;
    return status;
}

// The tokens between two blocks: from `pos`, the token after block p's subtree (p < 0: from the root, pos 0), the nodes
// above depth Dc in preorder up to the next block root the stream holds, which must be where the table says, or to the
// end of the stream, which must be numActive.  Every block below a node pruned on the way must be dead in the table.
// With index_block_walk over every live block and this after each of them and from the root, every token of the stream
// is parsed exactly once.  Returns 0, -1 (the stream ends inside the tree), -3 (tokens left over) or -4 (the table
// disagrees with the stream).  Reads tokens below numActive and the table; writes nothing.
VR_HD inline int block_gap_walk(const uint32_t *W, uint32_t numActive, int Dc, const uint32_t *blockOff, int64_t p, uint32_t pos)
{
    int j = 0;
    uint32_t path = 0;
    if (p >= 0) {
        j = Dc; path = (uint32_t)p;
        while (j > 0 && (path & 1u)) { path >>= 1; --j; }
        if (j == 0) return pos == numActive ? 0 : -3;
        path |= 1u;
    }
    while (true) {
        if (j == Dc) return blockOff[path] == pos ? 0 : -4;
        if (pos >= numActive) return -1;
        if (wget(W, pos++) == 3) {
            for (uint32_t i = path << (Dc - j), e = (path + 1u) << (Dc - j); i < e; ++i) if (blockOff[i] != VR_IDX_DEAD) return -4;
            while (j > 0 && (path & 1u)) { path >>= 1; --j; }
            if (j == 0) return pos == numActive ? 0 : -3;
            path |= 1u;
        } else { ++j; path <<= 1; }
    }
}

// ---- installing streams (capi.hip vr_brickset_set_tree / _set_trees execute it; they decide nothing) ----
// Every refusal and every buffer of an install from plain inputs.  Two engines fill a brick's decode index: the host
// parse of vr_brickset_set_tree (build_index_from_stream, uploaded) and kd_index.hip's kernels behind
// vr_brickset_set_trees, from a block table that is the caller's (block_table_ok checks it) or made here
// (block_table_from_stream).  Contract with capi.hip: everything in `needs` exists (ensure_install_buffers) before the
// first write to the set or to device memory.

// The grown-branch distances as the reference writes them (R.cpp:94-97), which the fine decoders hold as constants: a
// brick whose map says otherwise gets no fine side-car and is decoded by the walking kernel, which reads the map
VR_HD inline bool std_chain_distances(const uint8_t *dmap, int D)
{
    bool ok = true;
    for (int i = 0; i < VR_CHAIN_LEVELS; ++i) ok = ok && dmap[D + 1 + i] == (uint8_t)(64 >> i);
    return ok;
}

// One stream against its set.  status: VR_OK or, in this order, VR_ERR_INVALID (a null stream or map, one table pointer
// without the other, a short map, no tokens), VR_ERR_UNSUPPORTED (2^32 tokens or more), VR_ERR_FORMAT (fewer bytes than
// the tokens take, or more than a stream slot holds).  need: the tokens' bytes; tail: the bytes zeroed behind them (the
// decoders read past a stream's last token, never further than VR_TREE_TAIL bytes: DESIGN.md 3.3).  Both 0 unless VR_OK.
struct StreamCheck { int status; int64_t need, tail; };
StreamCheck check_stream(int maxDepth, int64_t treeCap, const vr_tree_desc &d);

enum class InstallEngine { HOST_PARSE, DEVICE_INDEX };      // vr_brickset_set_tree / vr_brickset_set_trees
enum class HostPass { BUILD_INDEX, TABLE_FROM_STREAM, TABLE_CHECK };    // build_index_from_stream / block_table_from_stream / block_table_ok
struct InstallInputs {
    int32_t D, Ds, K, B, maxDepth, variant;
    int64_t nIdx, treeCap;
    bool idx64, built, foreign;
    InstallEngine engine;
    int32_t count;
    const int32_t *bricks;          // count
    const vr_tree_desc *descs;      // count
};
struct InstallNeeds { bool idxTop, instOff, instFlag, instList, fineIdx, idxVal3, idxBase; };   // beyond what vr_brickset_create makes
struct InstallBrick { int64_t need, tail; bool fineOk; HostPass pass; };    // fineOk: wantFine and a map of the standard distances
struct InstallPlan {
    // VR_OK or the call's refusal (then nothing below `wantFine` is filled in).  DEVICE_INDEX: a null list or a count
    // outside 1 .. B (INVALID), a MidRangeTree set or 64-bit offsets (UNSUPPORTED), a built set (STATE), then stream by
    // stream: a brick out of range or named twice (INVALID), check_stream.  HOST_PARSE: the same per stream, but a built
    // set's STATE comes behind a stream's INVALID and UNSUPPORTED and in front of its FORMAT, and no variant is refused.
    int status;
    bool firstInstall;              // a fresh set: the whole set goes to "never installed" first
    int64_t nBlk;                   // blocks per brick, 2^block_depth(D)
    bool wantFine;                  // the set's geometry has the fine side-car (K == 6 and D >= 6)
    std::vector<InstallBrick> brick;    // per named brick
    InstallNeeds needs;
};
InstallPlan make_install_plan(const InstallInputs &in);
// a named brick's BrickSet::fineHas when the call ends.  failed: the device found a stream of the call outside the
// grammar, and every named brick is left never installed (no counts are read: 1)
inline uint8_t install_fine_has(const InstallBrick &b, bool failed) { return failed || b.fineOk ? 1 : 0; }

// ---- the brick-set archive (layout: vrhip.h "compressed brick-set archives"); parsing and writing need no device ----
constexpr int VR_ARCHIVE_HEADER_BYTES = 64, VR_ARCHIVE_ENTRY_BYTES = 32;
struct ArchiveGeom { int32_t variant; int64_t dims[3]; int32_t numBricks, D, maxDepth; };
struct ArchiveEntry { int64_t offset, treeBytes, numActive; uint64_t hash; };      // as it lies in the file
static_assert(sizeof(ArchiveEntry) == VR_ARCHIVE_ENTRY_BYTES, "the directory is read as it lies in memory");
struct ArchiveRecord { const uint8_t *dmap, *topVal; const uint32_t *blockOff; const uint8_t *tree; };
struct ArchiveBrick { int64_t numActive = 0; const uint8_t *dmap = nullptr, *tree = nullptr; std::vector<uint32_t> blockOff; std::vector<uint8_t> topVal; };
uint64_t fnv1a64(const uint8_t *p, int64_t n);
int64_t archive_record_bytes(int D, int maxDepth, int64_t treeBytes);
// 0, or -1: a wrong magic or version, a header that does not describe a brick set, an offset or length outside the
// blob, a record whose checksum or block table is wrong.  blob: 4-byte aligned
int archive_parse(const void *blob, int64_t bytes, ArchiveGeom &g, std::vector<ArchiveEntry> &dir);
ArchiveRecord archive_record(const void *blob, const ArchiveGeom &g, const ArchiveEntry &e);
// bricks[b].numActive == 0: brick b is absent
bool archive_write(FILE *f, const ArchiveGeom &g, const std::vector<ArchiveBrick> &bricks);
// workers for the host passes of an archive (checksums, tables): at most 16, never the machine's core count
void parallel_for(int n, const std::function<void(int)> &fn);

// ---- the file header of VolumeKdtree::save (R.cpp:535-544) and MidRangeTree::save (M.cpp:753-785) ----
struct Header { int64_t rootMin[3], rootMax[3]; int32_t maxDepth, origDepth; int64_t X, Y, Z, numActive; };
constexpr int VR_HEADER_BYTES = 88;
static_assert(sizeof(Header) == VR_HEADER_BYTES, "the header is written as it lies in memory");
// false: short read, maxDepth outside [VR_CHAIN_LEVELS, VR_MAX_DEPTH) or numActive <= 0
bool read_header(FILE *f, Header &h);
bool write_header(FILE *f, const Header &h);

} // namespace vr
