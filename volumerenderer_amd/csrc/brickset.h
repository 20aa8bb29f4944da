// brickset.h -- host-side state behind the opaque vr_brickset handle.
#pragma once
#include "kd_common.h"
#include "../../include/vrhip.h"
#include <algorithm>
#include <string>
#include <vector>

namespace vr {

struct Stream2 {              // one 2-bit stream (mid, or MidRangeTree's half-range stream)
    uint8_t *temp = nullptr;  // B * heapStride   truth heap (midrange / half range), 1-based
    uint8_t *codes = nullptr; // B * codeStride   2-bit codes, four per byte (TwoBitArray packing), 1-based heap (BFS)
    uint8_t *recon[3] = {nullptr, nullptr, nullptr}; // B * reconStride each: parents + two level buffers
    Ctrl *ctrl = nullptr;     // B
    uint8_t *tree = nullptr;  // B * treeCap      the stream the decoders read: the reference's contiguous preorder stream (TwoBitArray
                              //                  packing) or, after a fused build, its block-gapped form (BrickSet::gapped)
    uint8_t *treeCompact = nullptr; // BrickSet::compactCap bytes: fused builds: the reference's contiguous streams, brick b at byte
                                    // BrickSet::brickOff[b] (compact_launch; at the end of build() unless compaction was turned off)
};

// vr_brickset_decode_lod: the device state of one call.  Calls take the slots of a ring in turn; a call waits on the
// host for its slot's previous call (its event) before rewriting anything in it, so up to VR_LOD_SLOTS calls of a set
// may be queued, on one stream or several, without a host synchronisation, and none overwrites what another still reads.
#define VR_LOD_SLOTS 4
struct LodSlot {
    int32_t *dev = nullptr;        // 3B: the cuts of all B bricks, then the class lists (together at most 2B entries)
    int32_t *host = nullptr;       // 3B pinned: the same, staged for the copy
    // (the next three: made by capi.hip ensure_lod_slot for the first call whose LodPlan::needs names them)
    uint8_t *idxValCut = nullptr;  // B * nIdx: cut values of the bricks cut above depth Ds
    uint32_t *decTables = nullptr; // B * VR_FD_TABLE_WORDS: k_decode_fine's tables at each brick's cut
    uint8_t *rankVals = nullptr;   // B * 2^D * 2: general-extent decode scratch
    int64_t *obDev = nullptr;      // 3B, pool decodes only: each list entry's output offset (B), then the pack
    int64_t *obHost = nullptr;     //   descriptors of the coarse bricks (2 per brick); 3B pinned: the same, staged
    vr_pool_entry *tabHost = nullptr;  // pool decodes with a table: its pinned host image (tabCap entries)
    int64_t tabCap = 0;
    hipEvent_t done = nullptr;     // recorded after the call's last launch
    bool pending = false;
};

struct BrickSet {
    int32_t B = 0;
    Switches sw;              // host_plan.h: one table, read from the environment once, at vr_brickset_create
    BuildPlan plan{};         // of the current build (vr_brickset_build, before its first launch): host_plan.h
    Geom g{};
    TilePlan tile{};          // launch geometry (host_plan.h), made once by vr_brickset_create: nothing in it depends on
    RegionPlan region{};      // the switches or on anything else that can change afterwards
    Pyr12Plan pyr12{};
    int32_t D = 0, maxDepth = 0;
    int32_t tolerance = 6, maxEpochs = 5, variant = 0;
    int32_t K = 0;            // decode index granularity: subtrees of 2^K leaves
    int32_t Ds = 0;           // D - K
    int64_t heapStride = 0;   // 2^(D+1)
    // After a SkipBlocks build (kd_encode.hip) parts of the truth heaps (Stream2::temp) are UNDEFINED -- whatever an
    // earlier build or the allocator left there: levels D-1 and D of every constant 4096-leaf block (blockFlag bit 0) of
    // a constant brick, and of every such block the level loop skipped (bit 1).  No kernel uses them (DESIGN.md 3.2,
    // "who loads levels D-1 and D"); a new reader must check Ctrl::constBrick and the flag first.
    int64_t leafStride = 0;   // 2^D
    int64_t codeStride = 0;   // bytes of packed BFS codes per brick: heapStride / 4, 4-byte aligned (leafless builds: the levels above the leaves only)
    int64_t reconStride = 0;  // bytes per brick of a reconstruction buffer: 2^D, or 2^(D-1) in a leafless build
    // A fused build (k_prune_emit12) never stores the leaf level's codes and reconstruction: its leaf-level fills only
    // sum errors, and the prune recomputes both from (truth, parent's reconstruction, the distances the level loop ended
    // with: Ctrl::finalReconDist / finalCodesDist).  Set from BuildPlan::leafless when the encoder's buffers are allocated.
    bool leafless = false;
    int64_t treeCap = 0;      // bytes per brick reserved for the preorder stream
    int64_t nIdx = 0;         // 2^Ds index entries per brick

    Stream2 mid, rng;
    uint8_t *mmMin[2] = {nullptr, nullptr}, *mmMax[2] = {nullptr, nullptr}; // pyramid carry arrays
    unsigned long long *blockErr = nullptr; // B * nErrBlk : per-block sum err^2 of the fill pass
    int64_t nErrBlk = 0;
    void *estSumm = nullptr;     // B * estSummStride EstSummary records (estimator, kd_encode.hip)
    int64_t estSummStride = 0;
    unsigned long long *blockL1 = nullptr; // B * nEmitBlk
    uint8_t *blockFlag = nullptr;          // B * 2^(D-12): kd_encode.hip SkipBlocks (constant / skipped 4096-leaf blocks)
    uint8_t *blockFlagR = nullptr;         // ... of a MidRangeTree's half-range stream
    uint8_t *blockAlive = nullptr, *blockVal = nullptr;   // B * nEmitBlk
    unsigned long long *blockSpine = nullptr, *blockSpineR = nullptr; // B * nEmitBlk (R: MidRangeTree's range stream)
    uint32_t *chainLut = nullptr;   // 256: grown branch of a leaf by its initial error (k_chain_lut)
    uint32_t *blockTot = nullptr, *blockOff = nullptr; // B * nEmitBlk
    bool idx64 = false;            // more than 2^32 tokens possible (origTreeDepth > 28; VRHIP_FORCE_IDX64=1 for tests): 64-bit scan,
    unsigned long long *blockOff64 = nullptr, *idxBase = nullptr;   // block-relative index entries + per-block bases (B * nEmitBlk each)
    int64_t nEmitBlk = 0;
    uint32_t *idxOff = nullptr; // B * nIdx  token offset of each depth-Ds subtree root (VR_IDX_DEAD: inside a pruned region)
    uint8_t *idxVal = nullptr;  // B * nIdx  decoded scalar of that root (or of the pruned ancestor)
    uint8_t *idxValCut = nullptr; // B * nIdx  progressive cut above the index level: ancestor scalars
    uint8_t *fineIdx = nullptr;   // B * nIdx * 16  tokens owned by each 4-leaf subtree of a depth-Ds node (fused encoder only)
    std::vector<uint8_t> fineHas; // per brick: fineIdx describes its current stream (all set -> k_decode_fine)
    bool fineAll = false;         // ... of every brick: kept by fine_has_changed() wherever fineHas is assigned
    uint32_t *decTables = nullptr; // B * FD_TABLE_WORDS: k_decode_fine's tables of every brick for the current cut
    uint8_t *idxVal3 = nullptr;   // B * nIdx * 8   decoded scalar of every depth-(D-3) node (k_decode_quad; with fineIdx)
    uint32_t *boxUniform = nullptr; // B * 2^(D-12)  1: every voxel of the 4096-leaf box decodes to one byte at every cut >= D-3 (written by
                                  // k_prune_emit12_const for the strings it composes; cleared by every build; k_decode_region's hint, with fineIdx)
    uint32_t *chainTab = nullptr; // 8 x 16384 entries: k_decode_quad's grown-branch tables, one per number of refining levels (0..7),
    bool chainTabReady = false;   // all written once (never rewritten: decodes of one set on several streams may share them)
    std::vector<std::vector<uint8_t>> hostTree; // foreign streams keep their bytes for progressive cuts
    // vr_brickset_set_trees (kd_index.hip): a brick it installed keeps no host bytes (its hostTree entry is empty); its
    // cuts above depth Ds come from idxTop.  All made by the first such call
    uint8_t *idxTop = nullptr;    // B * 2 nIdx: 1-based heap of the decoded scalars of depths 0 .. Ds (host_plan.h "block tables")
    uint32_t *instOff = nullptr;  // B * 2^Dc: the block tables' offsets, as installed
    int32_t *instFlag = nullptr;  // B: a call's grammar flags, per named row
    int32_t *instList = nullptr;  // B: a call's named bricks
    uint32_t *lut = nullptr;    // 2^K : local rank -> packed (dx | dy<<10 | dz<<20)
    bool foreignRange = false;   // a foreign MidRangeTree file also supplied the range stream
    uint32_t *spread = nullptr;  // rank bits of every x, y, z coordinate: rank(x,y,z) = spread[x] | spread[X+y] | spread[X+Y+z]
    // General extents (any axis not a power of two, or longer than 1024): the reference's split rule (R.cpp:151-162)
    // then gives boxes of unequal size, an axis order that differs from node to node, leaves that span two cells or
    // none.  The tree itself is still the complete binary heap of 2^D leaves, so every rank-domain kernel (level loop,
    // prune, emit, stream parse) runs unchanged; only the two ends that touch voxels go through tables:
    bool generalGeom = false;
    uint32_t *srcIdx = nullptr;    // 2^D: voxel a leaf reads, the min corner of its build box (R.cpp:194-195)
    uint32_t *ownerRank = nullptr; // X*Y*Z: the leaf whose decoded value a voxel ends up with: the last one in preorder
                                   // whose levelCut box covers it (R.cpp:759-766, 790-799, 821-830)
    uint8_t *ownerSurv = nullptr;  // X*Y*Z: how many halvings of its leaf's box along a grown branch the voxel survives
    uint8_t *rankVals = nullptr;   // B * 2^D * 2: decoded value | branch nodes << 8 of every leaf rank (general-extent decode scratch)

    std::vector<Ctrl> hostCtrl; // copied back lazily
    std::vector<int32_t> hostRevertsR;   // MidRangeTree: reverted epochs of the half-range stream, per brick (sync_ctrl)
    uint32_t lutZeroRun = 0;    // chainLut[256]: table entries that would need the zero-run rewrite (always 0)
    bool encoderReady = false;  // every buffer of ensure_encoder_buffers (capi.hip) is allocated
    bool built = false, hostCtrlValid = false;
    bool gapped = false;        // mid.tree / rng.tree hold 4096-leaf block strings in fixed slots (kd_encode.hip PE_WORDS)
    bool compactValid = false;  // treeCompact holds the current build's contiguous stream (unless compactOverflow says it did not fit)
    bool compactOnBuild = true; // build() ends with the contiguous stream, like the reference's (tree.swap(preorderTree), R.cpp:714-718)
    int64_t compactCap = 0;     // bytes of each treeCompact buffer: sized from the streams' real lengths, not from their worst case
    unsigned long long *brickOff = nullptr;   // B + 1 (device): byte offset of every brick's stream in treeCompact (16-byte aligned); [B] = total
    int32_t *compactOverflow = nullptr;       // device flag: the streams did not fit compactCap (nothing was written; the host regrows and repeats)
    std::vector<unsigned long long> hostBrickOff;
    bool foreign = false;       // stream installed by set_tree/open (no encoder state)
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // MidRangeTree: the half-range stream's level loop runs on a stream of its own beside the mid stream's (fork / join
    // by events around the two compress_stream calls), with its own partial-sum and estimator scratch
    hipStream_t aux = nullptr, auxN[3] = {nullptr, nullptr, nullptr};     // aux == auxN[0]
    hipEvent_t evFork = nullptr, evJoin = nullptr, evJoinN[3] = {nullptr, nullptr, nullptr};
    int levelLoopStreams = 2;      // VolumeKdtree: brick ranges whose level loops run side by side (1 = none); vr_brickset_set_concurrency
    unsigned long long *blockErrR = nullptr;
    void *estSummR = nullptr;
    float phasesMs[5] = {0, 0, 0, 0, 0};
    bool timingsPending = false, decodeTimingPending = false;
    void *lastStream = nullptr;
    LodSlot lodSlot[VR_LOD_SLOTS];
    int lodNext = 0;
    // vr_brickset_decode_lod_pool: VR_POOL_STAGE_BRICKS decoded coarse bricks (ensure_lod_slot, for the first staged plan), shared by the calls of
    // every stream; stageDone is recorded after a call's last read of it and waited for by the next call's stream
    uint8_t *poolStage = nullptr;
    hipEvent_t stageDone = nullptr;
    bool stagePending = false;
    // vr_brickset_error_table: (maxDepth + 1) rows of B entries (first needed); a call clears the rows it fills on its
    // stream and synchronises that stream before it returns, so no two calls ever share it
    vr_brick_error *errTable = nullptr;
};

// vr_brickset_decode_lod_pool's destinations (vr_lod_pool_layout, computed by the caller): brick b with cut >= 0 goes
// to pool + off[b], shift[3b .. 3b+2] as in vr_pool_entry; the table (if tabDev) is uploaded from tab
struct PoolDest {
    uint8_t *pool = nullptr;
    const int64_t *off = nullptr;
    const uint8_t *shift = nullptr;
    const vr_pool_entry *tab = nullptr;
    vr_pool_entry *tabDev = nullptr;
    int64_t cells = 0;
};

// The tolerance the kernels get.  A leaf error never exceeds 255, so every tolerance >= 256 means the same thing; the
// fused prune kernels carry it in two signed 16-bit lanes (kd_encode.hip pe_leaf_table), which the caller's value
// (any non-negative int32) would overflow from 32769 up.
inline int kernel_tolerance(const BrickSet &b) { return b.tolerance < 256 ? b.tolerance : 256; }

inline void fine_has_changed(BrickSet &b) { b.fineAll = (int)b.fineHas.size() == b.B && std::find(b.fineHas.begin(), b.fineHas.end(), 0) == b.fineHas.end(); }

// kd_encode.hip
// executes the plan: allocates nothing, creates no stream or event (capi.hip vr_brickset_build has made whatever the plan touches)
int encode_launch(BrickSet *bs, const BuildPlan &plan, const uint8_t *voxDev, hipStream_t st);
// fused builds: contiguous stream(s) into Stream2::treeCompact; -1 without its buffers (capi.hip ensure_compact_buffers)
int compact_launch(BrickSet *bs, hipStream_t st);
// kd_decode.hip
// execute a plan (host_plan.h): allocate nothing, create no event; capi.hip has made whatever the plan's `needs` names,
// written the quad tables (chain_tables_launch, once per set) and filled the cut values a foreign set's plan leaves to it
int chain_tables_launch(BrickSet *bs, hipStream_t st);
int decode_launch(BrickSet *bs, const DecodePlan &plan, uint8_t *outDev, hipStream_t st);
// per-brick cuts: lod_stage uploads the plan's lists, offsets and pool table through the slot the caller has claimed,
// decode_lod_launch runs the classes (outDev: the caller's buffer, the pool of a pool decode) and records the slot's event
int lod_stage(BrickSet *bs, const LodPlan &plan, LodSlot &slot, const vr_pool_entry *tab, vr_pool_entry *tabDev, hipStream_t st);
int decode_lod_launch(BrickSet *bs, const LodPlan &plan, LodSlot &slot, uint8_t *outDev, hipStream_t st);
void free_lod_slots(BrickSet *bs);
// error_table.hip: per-brick error of two buffers of B bricks x V bytes, added into out[0 .. B) (cleared by the caller)
int brick_error_launch(const uint8_t *a, const uint8_t *b, int64_t B, int64_t V, vr_brick_error *out, hipStream_t st);
// kd_index.hip: the index of installed streams, rebuilt on the device.  Each enqueues on st and returns 0 or -1.
// resets the index entries of the n listed bricks (list null: of bricks 0 .. n-1) to "never installed"; onlyFlagged:
// of those whose flag is set (flags null: of all of them), with their scalar heaps and control blocks' token counts
int index_reset_launch(BrickSet *bs, const int32_t *listDev, int n, const int32_t *flagsDev, bool onlyFlagged, hipStream_t st);
int index_from_stream_launch(BrickSet *bs, const int32_t *listDev, int n, int32_t *flagsDev, hipStream_t st);
// out[brick][path] = idxTop[brick][(1 << cut) + (path >> (Ds - cut))] for the n listed bricks (list null: bricks
// first .. first + n - 1 at `cut`; else each at cuts[brick])
int cut_from_top_launch(BrickSet *bs, const int32_t *listDev, const int32_t *cutsDev, int first, int n, int cut, uint8_t *out,
                        hipStream_t st);
// does brick br take its cuts above depth Ds from idxTop (installed by vr_brickset_set_trees)?
inline bool top_indexed(const BrickSet &b, int br) { return b.idxTop && ((size_t)br >= b.hostTree.size() || b.hostTree[(size_t)br].empty()); }
int build_general_geometry(BrickSet *bs);   // srcIdx / ownerRank for general extents (0, -3 out of memory, -1 device error)

} // namespace vr
