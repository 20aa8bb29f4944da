// capi.hip -- the extern "C" boundary declared in include/vrhip.h.  Thin: argument
// checks, device memory management, launches (kd_encode/kd_decode/raymarch.hip) and
// the reference's file format.  No CPU compute path exists behind these entry points.
#include "../../include/vrhip.h"
#include "brickset.h"
#include "raymarch.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <atomic>
#include <map>
#include <mutex>
#include <new>

using namespace vr;

struct vr_brickset { BrickSet s; };

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_ == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_NO_DEVICE; } while (0)

static bool device_ok()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if ((e != hipSuccess || n <= 0) && getenv("VRHIP_DEBUG"))
        fprintf(stderr, "[vrhip] hipGetDeviceCount: %s (n=%d)\n", hipGetErrorString(e), n);
    return e == hipSuccess && n > 0;
}

// first need: a device / pinned host buffer that stays (false: it could not be made)
template <class T> static bool ensure_dev(T *&p, size_t bytes) { return p || hipMalloc(&p, bytes) == hipSuccess; }
template <class T> static bool ensure_pinned(T *&p, size_t bytes) { return p || hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess; }

// a vr_projection (vrhip.h); vr_compositor_composite_proj (compositor.hip) makes the same check through raymarch.h
namespace vr {
bool projection_ok(const vr_projection *pj)
{
    if (!pj || pj->op < VR_PROJECT_MAX || pj->op > VR_PROJECT_MEAN) return false;
    if (!isfinite(pj->window_lo) || !isfinite(pj->window_hi) || !(pj->window_hi > pj->window_lo)) return false;
    for (int k = 0; k < 3; ++k) if (!isfinite(pj->background[k])) return false;
    return ((uintptr_t)pj->lut_dev & 15u) == 0u;
}
}

extern "C" {

vr_status vr_device_count(int32_t *count)
{
    if (!count) return VR_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return VR_OK;
}

vr_status vr_set_device(int32_t device)
{
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    HIPCHK(hipSetDevice(device));
    return VR_OK;
}

const char *vr_status_string(vr_status s)
{
    switch (s) {
    case VR_OK: return "ok";
    case VR_ERR_INVALID: return "invalid argument";
    case VR_ERR_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
    case VR_ERR_OOM: return "out of device memory";
    case VR_ERR_IO: return "file error";
    case VR_ERR_STATE: return "wrong state (no tree built / loaded)";
    case VR_ERR_FORMAT: return "malformed tree stream";
    case VR_ERR_UNSUPPORTED: return "unsupported dimensions or option";
    default: return "unknown";
    }
}

const char *vr_version(void) { return "vrhip 0.1 (gfx950)"; }

vr_status vr_malloc(void **dev, int64_t bytes)
{
    if (!dev || bytes <= 0) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    HIPCHK(hipMalloc(dev, (size_t)bytes));
    return VR_OK;
}
vr_status vr_free(void *dev)
{
    if (dev) hipFree(dev);
    return VR_OK;
}
vr_status vr_upload(void *dst, const void *src, int64_t bytes, void *stream)
{
    if (!dst || !src || bytes <= 0) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VR_OK;
}
vr_status vr_download(void *dst, const void *src, int64_t bytes, void *stream)
{
    if (!dst || !src || bytes <= 0) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VR_OK;
}

static void free_stream2(Stream2 &s)
{
    hipFree(s.treeCompact);
    hipFree(s.temp); hipFree(s.codes);
    for (int i = 0; i < 3; ++i) hipFree(s.recon[i]);
    hipFree(s.ctrl); hipFree(s.tree);
    s = Stream2();
}

// (the encoder's arrays are made by ensure_encoder_buffers at the first build)
static vr_status alloc_stream2(BrickSet &b, Stream2 &s)
{
    const size_t B = (size_t)b.B;
    HIPCHK(hipMalloc(&s.ctrl, B * sizeof(Ctrl)));
    HIPCHK(hipMemset(s.ctrl, 0, B * sizeof(Ctrl)));
    HIPCHK(hipMalloc(&s.tree, B * (size_t)b.treeCap));
    return VR_OK;
}

// everything ensure_encoder_buffers allocates (an opened MidRangeTree file owns rng.ctrl / rng.tree: kept)
static void free_encoder_buffers(BrickSet &b)
{
    auto drop = [](auto *&p) { if (p) hipFree(p); p = nullptr; };
    Stream2 *ss[2] = {&b.mid, &b.rng};
    for (Stream2 *s : ss) {
        drop(s->temp); drop(s->codes);
        for (int i = 0; i < 3; ++i) drop(s->recon[i]);
    }
    for (int i = 0; i < 2; ++i) { drop(b.mmMin[i]); drop(b.mmMax[i]); }
    drop(b.blockErr); drop(b.estSumm); drop(b.blockErrR); drop(b.estSummR); drop(b.blockL1); drop(b.blockFlag); drop(b.blockFlagR); drop(b.blockAlive); drop(b.blockVal); drop(b.blockSpine); drop(b.blockSpineR);
    drop(b.chainLut); drop(b.blockTot); drop(b.blockOff); drop(b.blockOff64); drop(b.idxBase);
    b.encoderReady = false;
}

static vr_status alloc_encoder_buffers(BrickSet &b, const BuildPlan &plan)
{
    const size_t B = (size_t)b.B;
    // a leafless build's codes and reconstruction arrays end one level above the leaves
    b.leafless = plan.leafless;
    b.reconStride = b.leafless ? b.leafStride / 2 : b.leafStride;
    b.codeStride = b.leafless ? b.leafStride / 4 + 16 : ((b.heapStride + 15) / 16) * 4;
    HIPCHK(hipMalloc(&b.mid.temp, B * (size_t)b.heapStride));
    HIPCHK(hipMalloc(&b.mid.codes, B * (size_t)b.codeStride));
    for (int i = 0; i < 3; ++i) HIPCHK(hipMalloc(&b.mid.recon[i], B * (size_t)b.reconStride));
    if (b.variant == VR_VARIANT_MIDRANGE) {
        if (!b.rng.ctrl) HIPCHK(hipMalloc(&b.rng.ctrl, B * sizeof(Ctrl)));       // (an opened MidRangeTree file has these already)
        if (!b.rng.tree) HIPCHK(hipMalloc(&b.rng.tree, B * (size_t)b.treeCap));
        HIPCHK(hipMalloc(&b.rng.temp, B * (size_t)b.heapStride));
        HIPCHK(hipMalloc(&b.rng.codes, B * (size_t)b.codeStride));
        for (int i = 0; i < 3; ++i) HIPCHK(hipMalloc(&b.rng.recon[i], B * (size_t)b.reconStride));
    }
    for (int i = 0; i < 2; ++i) {
        HIPCHK(hipMalloc(&b.mmMin[i], B * (size_t)plan.rootStride));
        HIPCHK(hipMalloc(&b.mmMax[i], B * (size_t)plan.rootStride));
    }
    b.nErrBlk = ((int64_t)1 << b.D) / 1024 > 0 ? ((int64_t)1 << b.D) / 1024 : 1;
    HIPCHK(hipMalloc(&b.blockErr, 3 * B * (size_t)b.nErrBlk * sizeof(unsigned long long)));     // + the central difference's two planes (Ctrl::altSel)
    b.estSummStride = ((int64_t)1 << b.D) / 1024 > 0 ? ((int64_t)1 << b.D) / 1024 : 1;
    HIPCHK(hipMalloc(&b.estSumm, B * (size_t)b.estSummStride * 128));
    if (b.variant == VR_VARIANT_MIDRANGE) {
        HIPCHK(hipMalloc(&b.blockErrR, 3 * B * (size_t)b.nErrBlk * sizeof(unsigned long long)));
        HIPCHK(hipMalloc(&b.estSummR, B * (size_t)b.estSummStride * 128));
    }
    HIPCHK(hipMalloc(&b.blockL1, B * (size_t)b.nEmitBlk * sizeof(unsigned long long)));
    // (BuildPlan's contract: the flags exist exactly when the build is fused, the range stream's for a MidRangeTree)
    if (plan.fused) HIPCHK(hipMalloc(&b.blockFlag, B * (size_t)plan.boxes));
    if (plan.fused && plan.midRange) HIPCHK(hipMalloc(&b.blockFlagR, B * (size_t)plan.boxes));
    HIPCHK(hipMalloc(&b.blockAlive, B * (size_t)b.nEmitBlk));
    HIPCHK(hipMalloc(&b.blockVal, B * (size_t)b.nEmitBlk));
    HIPCHK(hipMalloc(&b.blockSpine, B * (size_t)b.nEmitBlk * sizeof(unsigned long long)));
    if (b.variant == VR_VARIANT_MIDRANGE) HIPCHK(hipMalloc(&b.blockSpineR, B * (size_t)b.nEmitBlk * sizeof(unsigned long long)));
    HIPCHK(hipMalloc(&b.chainLut, (260 + 512) * sizeof(uint32_t)));   // 256 entries + [256]: entries that would need the zero-run rewrite; + 512 keyed by the signed error
    HIPCHK(hipMalloc(&b.blockTot, B * (size_t)b.nEmitBlk * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&b.blockOff, B * (size_t)b.nEmitBlk * sizeof(uint32_t)));
    if (b.idx64) {
        HIPCHK(hipMalloc(&b.blockOff64, B * (size_t)b.nEmitBlk * sizeof(unsigned long long)));
        if (!b.idxBase) HIPCHK(hipMalloc(&b.idxBase, B * (size_t)b.nEmitBlk * sizeof(unsigned long long)));    // (set_tree may have made it)
    }
    return VR_OK;
}

// "ready" is a flag of its own, set after the last allocation: a failure part-way (out of memory) releases what
// was taken, so the next build retries from scratch and reports the same error instead of launching kernels on
// null side buffers.
static vr_status ensure_encoder_buffers(BrickSet &b, const BuildPlan &plan)
{
    if (b.encoderReady) return VR_OK;
    const vr_status rc = alloc_encoder_buffers(b, plan);
    if (rc != VR_OK) { (void)hipGetLastError(); free_encoder_buffers(b); return rc; }
    b.encoderReady = true;
    return VR_OK;
}

// What a fused build writes beside the encoder's arrays: the fine index, the depth-(D-3) scalars and the uniform hint
static vr_status ensure_fused_buffers(BrickSet &b, const BuildPlan &plan)
{
    const size_t B = (size_t)b.B;
    if (!b.fineIdx) HIPCHK(hipMalloc(&b.fineIdx, B * (size_t)b.nIdx * 16));
    if (!b.idxVal3) HIPCHK(hipMalloc(&b.idxVal3, B * (size_t)b.nIdx * 8));
    if (!b.boxUniform) HIPCHK(hipMalloc(&b.boxUniform, B * (size_t)plan.boxes * sizeof(uint32_t)));
    return VR_OK;
}

// The buffers of compact_launch (kd_encode.hip): brickOff, compactOverflow and a treeCompact of at least minCap bytes
// per stream the variant has (0: whatever there is, or the first guess), for the build and for contiguous_stream's
// regrow.  compactCap is non-zero only while every treeCompact the variant needs exists: it is cleared before anything
// is freed and assigned after the last allocation.
static vr_status ensure_compact_buffers(BrickSet &b, int64_t minCap)
{
    if (!b.brickOff) HIPCHK(hipMalloc(&b.brickOff, (size_t)(b.B + 1) * sizeof(unsigned long long)));
    if (!b.compactOverflow) HIPCHK(hipMalloc(&b.compactOverflow, sizeof(int32_t)));
    if (b.compactCap != 0 && b.compactCap >= minCap) return VR_OK;
    int64_t cap = minCap;
    if (cap == 0) {
        // first time: 5/8 byte per voxel (the bench volume takes 0.56; noise takes up to 2.3) -- a guess, corrected on demand
        cap = (int64_t)b.B * b.g.voxels / 8 * 5 + (int64_t)b.B * 64 + 4096;
        cap = std::min(cap, (int64_t)b.B * b.treeCap);
    }
    b.compactCap = 0;
    b.compactValid = false;
    hipFree(b.mid.treeCompact); b.mid.treeCompact = nullptr;
    hipFree(b.rng.treeCompact); b.rng.treeCompact = nullptr;
    HIPCHK(hipMalloc(&b.mid.treeCompact, (size_t)cap));
    if (b.variant == VR_VARIANT_MIDRANGE && hipMalloc(&b.rng.treeCompact, (size_t)cap) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(b.mid.treeCompact); b.mid.treeCompact = nullptr;
        return VR_ERR_OOM;
    }
    b.compactCap = cap;
    return VR_OK;
}

// Internal streams for the forks of a build (kd_encode.hip encode_launch), created on first need and only as many as are
// used: a process has few hardware queues (4 by default), streams beyond them share one, and a kernel queued behind
// another stream's long copy on a shared queue waits for it (a MidRangeTree build inside the timestep streamer took 236
// instead of 68 ms with three idle extra streams per handle).  Returns how many of the n the handle has.
static int ensure_aux(BrickSet &b, int n)
{
    if (n > 3) n = 3;
    if (n <= 0) return 0;
    if (!b.evFork && hipEventCreateWithFlags(&b.evFork, hipEventDisableTiming) != hipSuccess) return 0;
    int have = 0;
    for (int i = 0; i < n; ++i) {
        if (!b.auxN[i] && hipStreamCreateWithFlags(&b.auxN[i], hipStreamNonBlocking) != hipSuccess) break;
        if (!b.evJoinN[i] && hipEventCreateWithFlags(&b.evJoinN[i], hipEventDisableTiming) != hipSuccess) break;
        ++have;
    }
    b.aux = b.auxN[0]; b.evJoin = b.evJoinN[0];
    return have;
}

// ---- a decode call, in the order of a build: validate, plan (host_plan.h make_decode_plan / make_lod_plan), check the
// caller's alignment from the plan, ensure every buffer its `needs` names (a per-brick call then waits for and claims its
// ring slot), fill the cut values the plan leaves to the caller, launch.  A failure up to the claim has enqueued nothing
// (but the quad tables, once per set), recorded no timing event and left the ring where it was.
static DecodeInputs decode_inputs(const BrickSet &b, bool rangeStream)
{
    DecodeInputs in{};
    in.D = b.D; in.Ds = b.Ds; in.B = b.B; in.nb0 = b.g.nb[0];
    in.nIdx = b.nIdx; in.voxels = b.g.voxels; in.leafStride = b.leafStride; in.nEmitBlk = b.nEmitBlk;
    in.generalGeom = b.generalGeom; in.idx64 = b.idx64;
    in.tileOk = b.tile.ok; in.tiles = b.tile.tilesX * b.tile.tilesY * b.tile.tilesZ;
    in.regionOk = b.region.ok; in.nreg = b.region.nreg;
    in.fineAll = b.fineIdx && b.fineAll; in.idxVal3 = b.idxVal3 != nullptr; in.foreign = b.foreign; in.rangeStream = rangeStream;
    in.decodeWalk = b.sw.decodeWalk; in.decodeFineV1 = b.sw.decodeFineV1; in.decodeQuad = b.sw.decodeQuad;
    in.noUniformDecode = b.sw.noUniformDecode;
    return in;
}

// k_decode_quad's tables, written once per set, by whichever call first needs them
static vr_status ensure_chain_tables(BrickSet &b, hipStream_t st)
{
    if (b.chainTabReady) return VR_OK;
    if (!ensure_dev(b.chainTab, (size_t)(VR_CHAIN_LEVELS + 1) * VR_QD_CHAIN_ENTRIES * 4)) return VR_ERR_OOM;
    // (the first use may come from any stream: make the tables visible to all of them before going on)
    if (chain_tables_launch(&b, st) != 0 || hipStreamSynchronize(st) != hipSuccess) return VR_ERR_NO_DEVICE;
    b.chainTabReady = true;
    return VR_OK;
}

// the scratch of a uniform decode (the set's) or of a per-brick one (its slot's); the quad tables last: nothing is
// enqueued before the last allocation
static vr_status ensure_decode_scratch(BrickSet &b, const DecodeNeeds &n, uint8_t *&idxValCut, uint32_t *&decTables, uint8_t *&rankVals,
                                       hipStream_t st)
{
    const size_t B = (size_t)b.B;
    if ((n.idxValCut && !ensure_dev(idxValCut, B * (size_t)b.nIdx)) || (n.decTables && !ensure_dev(decTables, B * VR_FD_TABLE_WORDS * 4)) ||
        (n.rankVals && !ensure_dev(rankVals, B * (size_t)b.leafStride * 2))) {
        (void)hipGetLastError();
        return VR_ERR_OOM;
    }
    return n.chainTab ? ensure_chain_tables(b, st) : VR_OK;
}

// The next ring slot with everything the plan touches, claimed (lodNext advances) only when all of it exists.  The
// slot's previous call (any stream) may still read its lists, cut values and tables: waited for first, on the host
static vr_status ensure_lod_slot(BrickSet &b, const LodPlan &p, hipStream_t st, LodSlot *&slot)
{
    LodSlot &s = b.lodSlot[b.lodNext];
    if (s.pending && hipEventSynchronize(s.done) != hipSuccess) return VR_ERR_NO_DEVICE;
    s.pending = false;
    const size_t B = (size_t)b.B;
    bool ok = ensure_dev(s.dev, 3 * B * sizeof(int32_t)) && ensure_pinned(s.host, 3 * B * sizeof(int32_t));
    if (!p.offsets.empty()) ok = ok && ensure_dev(s.obDev, 3 * B * sizeof(int64_t)) && ensure_pinned(s.obHost, 3 * B * sizeof(int64_t));
    if (ok && s.tabCap < p.tableCells) {
        if (s.tabHost) hipHostFree(s.tabHost);
        s.tabHost = nullptr; s.tabCap = 0;
        ok = ensure_pinned(s.tabHost, (size_t)p.tableCells * sizeof(vr_pool_entry));
        if (ok) s.tabCap = p.tableCells;
    }
    if (p.staged) ok = ok && ensure_dev(b.poolStage, (size_t)VR_POOL_STAGE_BRICKS * b.g.voxels);
    if (!ok) { (void)hipGetLastError(); return VR_ERR_OOM; }
    if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) return VR_ERR_NO_DEVICE;
    if (p.staged && !b.stageDone && hipEventCreateWithFlags(&b.stageDone, hipEventDisableTiming) != hipSuccess) return VR_ERR_NO_DEVICE;
    const vr_status rc = ensure_decode_scratch(b, p.needs, s.idxValCut, s.decTables, s.rankVals, st);
    if (rc != VR_OK) return rc;
    b.lodNext = (b.lodNext + 1) % VR_LOD_SLOTS;
    slot = &s;
    return VR_OK;
}

vr_status vr_brickset_destroy(vr_brickset *h)
{
    if (!h) return VR_OK;
    BrickSet &b = h->s;
    free_lod_slots(&b);
    hipFree(b.errTable);
    free_encoder_buffers(b);
    free_stream2(b.mid);
    free_stream2(b.rng);
    hipFree(b.brickOff); hipFree(b.compactOverflow);
    hipFree(b.idxTop); hipFree(b.instOff); hipFree(b.instFlag); hipFree(b.instList);
    hipFree(b.idxOff); hipFree(b.idxVal); hipFree(b.idxValCut); hipFree(b.fineIdx); hipFree(b.idxVal3); hipFree(b.boxUniform); hipFree(b.chainTab); hipFree(b.decTables); hipFree(b.lut); hipFree(b.spread); hipFree(b.srcIdx); hipFree(b.ownerRank); hipFree(b.ownerSurv); hipFree(b.rankVals);
    for (int i = 0; i < 8; ++i) if (b.ev[i]) hipEventDestroy(b.ev[i]);
    if (b.evFork) hipEventDestroy(b.evFork);
    for (int i = 0; i < 3; ++i) { if (b.evJoinN[i]) hipEventDestroy(b.evJoinN[i]); if (b.auxN[i]) hipStreamDestroy(b.auxN[i]); }
    delete h;
    return VR_OK;
}

static bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// vrhip.h "alignment of caller buffers": a call that would launch a kernel with vector accesses to a caller's buffer
// is refused, before anything is launched, unless that buffer is 16-byte aligned
static bool misaligned16(const void *p) { return ((uintptr_t)p & 15) != 0; }

vr_status vr_brickset_create(vr_brickset **out, int32_t num_bricks, const int64_t dims[3], int32_t tolerance,
                             int32_t max_epochs, int32_t variant)
{
    if (!out || !dims || num_bricks <= 0) return VR_ERR_INVALID;
    if (tolerance < 0 || max_epochs < 0 || variant < 0 || variant > 2) return VR_ERR_INVALID;
    for (int k = 0; k < 3; ++k) if (dims[k] <= 0) return VR_ERR_INVALID;
    if (max_epochs > VR_MAX_EPOCHS) return VR_ERR_UNSUPPORTED;   // the level loop's launches grow with it, whatever the data does
    // power-of-two extents up to 1024 per axis take the tiled kernels; anything else (the reference accepts any
    // extents, R.cpp:26-36,151-162) goes through the general-extent tables.  Limits: origTreeDepth <= 31, fewer than
    // 2^32 voxels per tree, and above depth 28 (64-bit token offsets) one tree per set.
    bool general = !pow2(dims[0]) || !pow2(dims[1]) || !pow2(dims[2]) || dims[0] > 1024 || dims[1] > 1024 || dims[2] > 1024;
    if (dims[0] > (1ll << 20) || dims[1] > (1ll << 20) || dims[2] > (1ll << 20) || dims[0] * dims[1] * dims[2] >= (1ll << 32))
        return VR_ERR_UNSUPPORTED;
    if (num_bricks > VR_MAX_BRICKS) return VR_ERR_UNSUPPORTED;   // the brick index rides on gridDim.y
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    vr_brickset *h = new (std::nothrow) vr_brickset();
    if (!h) return VR_ERR_OOM;
    BrickSet &b = h->s;
    b.B = num_bricks;
    b.sw = switches_from_env();      // the VRHIP_* debugging switches are read here, once per set (host_plan.h Switches)
    make_geom(b.g, dims);
    b.D = b.g.D;
    if (b.D > 31) { delete h; return VR_ERR_UNSUPPORTED; }
    // deeper than 28 (the reference's own 2048x2048x768 tree is 31 deep, main.cpp:242-251): a stream can pass 2^32
    // tokens, so the emitter scans in 64 bits and the decode index goes block-relative; table-driven geometry only
    b.idx64 = b.D > 28 || (getenv("VRHIP_FORCE_IDX64") && b.D >= 12);      // (create-time only, like the switches above)
    if (b.idx64) general = true;       // the tiled decoders read absolute 32-bit index entries
    if (b.idx64 && num_bricks != 1 && b.D > 28) { delete h; return VR_ERR_UNSUPPORTED; }
    b.generalGeom = general;
    b.maxDepth = b.D + VR_CHAIN_LEVELS;
    b.tolerance = tolerance; b.maxEpochs = max_epochs; b.variant = variant;
    b.K = b.D < 6 ? b.D : 6;   // decode index granularity: 4x4x4 voxel subtrees
    b.Ds = b.D - b.K;
    b.heapStride = (int64_t)1 << (b.D + 1);
    b.leafStride = (int64_t)1 << b.D;
    b.codeStride = ((b.heapStride + 15) / 16) * 4;     // (both final when the encoder's buffers are made: alloc_encoder_buffers)
    b.reconStride = b.leafStride;
    const int64_t numMax = b.heapStride - 1 + VR_CHAIN_LEVELS * b.leafStride; // numMaxNodes R.cpp:35
    b.treeCap = ((numMax + 15) / 16 + 2) * 4 + 256;   // slack: the decoder stages whole words past a run's end
    if (build_fused(b.D)) {   // a fused build keeps every 4096-leaf block's string in a fixed slot of 2320 words (kd_encode.hip PE_WORDS)
        const int64_t gappedBytes = ((int64_t)1 << (b.D - 12)) * 2320 * 4 + 256;
        if (gappedBytes > b.treeCap) b.treeCap = gappedBytes;
    }
    b.nIdx = (int64_t)1 << b.Ds;
    b.nEmitBlk = (b.leafStride + 255) / 256;
    make_plans(b.g, b.K, b.generalGeom, b.idx64, b.treeCap, b.tile, b.region, b.pyr12);
    vr_status rc = alloc_stream2(b, b.mid);
    if (rc == VR_OK) {
        hipError_t e = hipMalloc(&b.idxOff, (size_t)b.B * b.nIdx * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&b.idxVal, (size_t)b.B * b.nIdx);
        if (e == hipSuccess) e = hipMalloc(&b.idxValCut, (size_t)b.B * b.nIdx);
        if (e == hipSuccess && general) {
            const int grc = build_general_geometry(&b);
            if (grc != 0) e = grc == -3 ? hipErrorOutOfMemory : hipErrorUnknown;
        }
        const auto upload = [](uint32_t *dst, const std::vector<uint32_t> &v) {
            return hipMemcpy(dst, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        };
        if (e == hipSuccess) e = hipMalloc(&b.lut, ((size_t)1 << b.K) * sizeof(uint32_t));
        if (e == hipSuccess && !general) e = upload(b.lut, make_lut(b.g, b.K));
        if (e == hipSuccess && !general) e = hipMalloc(&b.spread, (size_t)(b.g.X + b.g.Y + b.g.Z) * sizeof(uint32_t));
        if (e == hipSuccess && !general) e = upload(b.spread, make_spread(b.g));
        for (int i = 0; i < 8 && e == hipSuccess; ++i) e = hipEventCreate(&b.ev[i]);
        // (the internal streams of a build are created when a build first needs them: ensure_aux)
        if (e != hipSuccess) rc = e == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_NO_DEVICE;
    }
    if (rc != VR_OK) { vr_brickset_destroy(h); return rc; }
    b.hostCtrl.resize(b.B);
    *out = h;
    return VR_OK;
}

vr_status vr_brickset_set_switch(vr_brickset *h, const char *name, int32_t value)
{
    if (!h || !name) return VR_ERR_INVALID;
    bool Switches::*const m = find_switch(name);
    if (!m) return VR_ERR_INVALID;
    h->s.sw.*m = value != 0;
    return VR_OK;
}

vr_status vr_brickset_set_compaction(vr_brickset *h, int32_t on_build)
{
    if (!h) return VR_ERR_INVALID;
    h->s.compactOnBuild = on_build != 0;
    return VR_OK;
}

vr_status vr_debug_set(const char *name, int32_t value)
{
    if (!name) return VR_ERR_INVALID;
    if (!strcmp(name, "skip_grid_v1")) { vr::g_skipGridV1.store(value ? 1 : 0); return VR_OK; }
    if (!strcmp(name, "reslice_tile_w")) {      // k_reslice's wave footprint: 8 x 8, 16 x 4 or 64 x 1 pixels
        if (value != 8 && value != 16 && value != 64) return VR_ERR_INVALID;
        vr::g_resliceTileLog2.store(value == 8 ? 3 : (value == 16 ? 4 : 6));
        return VR_OK;
    }
    if (!strcmp(name, "hist_plain")) { vr::g_histPlain.store(value ? 1 : 0); return VR_OK; }
    if (!strcmp(name, "mesh_count_only")) { vr::g_meshCountOnly.store(value ? 1 : 0); return VR_OK; }
    return VR_ERR_INVALID;
}

vr_status vr_brickset_set_error_tolerance(vr_brickset *h, int32_t tol)
{
    if (!h || tol < 0) return VR_ERR_INVALID;
    h->s.tolerance = tol;
    return VR_OK;
}
vr_status vr_brickset_set_max_epochs(vr_brickset *h, int32_t e)
{
    if (!h || e < 0) return VR_ERR_INVALID;
    if (e > VR_MAX_EPOCHS) return VR_ERR_UNSUPPORTED;      // (the set keeps its previous setting)
    h->s.maxEpochs = e;
    return VR_OK;
}

vr_status vr_brickset_build(vr_brickset *h, const uint8_t *vox, void *stream)
{
    if (!h || !vox) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    // k_pyramid12 serves the set: 16-byte loads from the caller's voxels
    if (b.pyr12.use12 && misaligned16(vox)) return VR_ERR_INVALID;
    // the side streams, then the plan (it takes how many there are), then every buffer its launches touch: a failure up
    // to here has enqueued nothing and changed nothing the previous build's readers use
    BuildInputs in{};
    in.D = b.D; in.B = b.B; in.variant = b.variant; in.tolerance = b.tolerance; in.maxEpochs = b.maxEpochs;
    in.use12 = b.pyr12.use12; in.lines = b.pyr12.lines; in.generalGeom = b.generalGeom;
    in.sw = b.sw; in.levelLoopStreams = b.levelLoopStreams; in.compactOnBuild = b.compactOnBuild;
    in.sideStreams = ensure_aux(b, build_side_streams(b.variant, b.B, b.levelLoopStreams));
    const BuildPlan plan = make_build_plan(in);
    vr_status rc = plan.fused ? ensure_fused_buffers(b, plan) : VR_OK;
    if (rc == VR_OK && plan.compact) rc = ensure_compact_buffers(b, 0);
    if (rc != VR_OK) { (void)hipGetLastError(); return rc; }
    // (vr_brickset_set_max_epochs(0) <-> >= 1 between two builds changes what the level loop keeps of the leaf level:
    // the encoder's arrays are made again for the other mode.  They are released first -- both sizes at once may not
    // fit -- and last of all buffers: if they cannot be made again the set has no build any more, VR_ERR_STATE from
    // then on, not kernels on null arrays)
    const bool resize = b.encoderReady && b.leafless != plan.leafless;
    if (resize) {
        HIPCHK(hipDeviceSynchronize());
        free_encoder_buffers(b);
    }
    rc = ensure_encoder_buffers(b, plan);
    if (rc != VR_OK) {
        if (resize) b.built = false;
        return rc;
    }
    b.hostCtrlValid = false;
    b.hostBrickOff.clear();
    b.foreign = false;
    b.plan = plan;
    if (encode_launch(&b, b.plan, vox, (hipStream_t)stream) != 0) return VR_ERR_NO_DEVICE;
    b.built = true;
    b.timingsPending = true;
    b.lastStream = stream;
    return VR_OK;
}

static vr_status sync_ctrl(BrickSet &b)
{
    if (!b.built) return VR_ERR_STATE;
    if (b.hostCtrlValid) return VR_OK;
    HIPCHK(hipStreamSynchronize((hipStream_t)b.lastStream));
    HIPCHK(hipMemcpy(b.hostCtrl.data(), b.mid.ctrl, (size_t)b.B * sizeof(Ctrl), hipMemcpyDeviceToHost));
    b.lutZeroRun = 0;
    if (b.chainLut && !b.foreign) HIPCHK(hipMemcpy(&b.lutZeroRun, b.chainLut + 256, sizeof(uint32_t), hipMemcpyDeviceToHost));
    // MidRangeTree: the half-range stream's level loop reverts epochs of its own (M.cpp:399-544)
    b.hostRevertsR.assign((size_t)b.B, 0);
    if (b.variant == VR_VARIANT_MIDRANGE && !b.foreign && b.rng.ctrl) {
        std::vector<Ctrl> r((size_t)b.B);
        HIPCHK(hipMemcpy(r.data(), b.rng.ctrl, (size_t)b.B * sizeof(Ctrl), hipMemcpyDeviceToHost));
        for (int i = 0; i < b.B; ++i) b.hostRevertsR[(size_t)i] = r[(size_t)i].constBrick ? 0 : r[(size_t)i].numReverts;
    }
    b.hostCtrlValid = true;
    return VR_OK;
}

vr_status vr_brickset_info(vr_brickset *h, int32_t brick, vr_tree_info *info)
{
    if (!h || !info || brick < 0 || brick >= h->s.B) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    vr_status rc = sync_ctrl(b);
    if (rc != VR_OK) return rc;
    const Ctrl &c = b.hostCtrl[brick];
    if (c.emitOverflow) return VR_ERR_STATE;   // internal count/emit mismatch: no valid stream
    memset(info, 0, sizeof(*info));
    info->X = b.g.X; info->Y = b.g.Y; info->Z = b.g.Z;
    info->orig_tree_depth = b.D;
    info->max_tree_depth = b.maxDepth;
    info->num_active_nodes = (int64_t)c.numActive;
    info->tree_bytes = ((int64_t)c.numActive + 3) / 4;
    info->tolerance = b.tolerance; info->max_epochs = b.maxEpochs; info->variant = b.variant;
    info->num_reverts = c.numReverts + ((size_t)brick < b.hostRevertsR.size() ? b.hostRevertsR[(size_t)brick] : 0);
    info->max_error_before = c.maxErrBefore;
    info->max_error_after = c.maxErrAfter;
    info->mean_l1_after = (double)c.statL1 / (double)b.leafStride;
    info->zero_run_rewrites = c.constBrick ? 0 : c.zeroRun + (int32_t)b.lutZeroRun;
    info->est_exact_segments = c.constBrick ? 0 : c.estFallbacks;
    return VR_OK;
}

// Device address of brick `brick`'s contiguous preorder stream (the reference's tree.bits) of stream s.  After a fused
// build the decoders read the block-gapped form; the reference's layout is in treeCompact, made at the end of build() or
// here, on demand.  Its buffers are sized from the streams' real lengths: when a build's streams did not fit (the first
// build of a set guesses; later ones may grow), the buffers are regrown to what is needed and the copy repeated.
static vr_status contiguous_stream(BrickSet &b, Stream2 &s, int brick, const uint8_t **ptr)
{
    if (!s.tree) return VR_ERR_STATE;
    if (!b.gapped) { *ptr = s.tree + (size_t)brick * b.treeCap; return VR_OK; }
    for (int attempt = 0; attempt < 2; ++attempt) {
        HIPCHK(hipStreamSynchronize((hipStream_t)b.lastStream));
        if (!b.compactValid) {
            const vr_status brc = ensure_compact_buffers(b, 0);
            if (brc != VR_OK) return brc;
            if (compact_launch(&b, (hipStream_t)b.lastStream) != 0) return VR_ERR_NO_DEVICE;
            HIPCHK(hipStreamSynchronize((hipStream_t)b.lastStream));
            b.hostBrickOff.clear();
        }
        if (b.hostBrickOff.size() != (size_t)b.B + 1) {
            b.hostBrickOff.resize((size_t)b.B + 1);
            HIPCHK(hipMemcpy(b.hostBrickOff.data(), b.brickOff, ((size_t)b.B + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            // (an emit overflow would have been flagged in the control blocks: re-read them)
            HIPCHK(hipMemcpy(b.hostCtrl.data(), b.mid.ctrl, (size_t)b.B * sizeof(Ctrl), hipMemcpyDeviceToHost));
            b.hostCtrlValid = true;
        }
        const int64_t total = (int64_t)b.hostBrickOff[(size_t)b.B];
        if (total <= b.compactCap) break;
        // did not fit: nothing was written.  Regrow (some headroom: the next timestep's streams differ) and repeat
        const vr_status brc = ensure_compact_buffers(b, total + total / 8 + 4096);
        if (brc != VR_OK) return brc;
        if (attempt == 1) return VR_ERR_STATE;
    }
    *ptr = s.treeCompact + (size_t)b.hostBrickOff[(size_t)brick];
    return VR_OK;
}

// the tokens' bytes of a brick's contiguous stream in a host vector (after sync_ctrl)
static vr_status download_stream(BrickSet &b, Stream2 &s, int brick, std::vector<uint8_t> &out)
{
    const uint8_t *src = nullptr;
    const vr_status rc = contiguous_stream(b, s, brick, &src);
    if (rc != VR_OK) return rc;
    out.resize((size_t)(((int64_t)b.hostCtrl[(size_t)brick].numActive + 3) / 4));
    HIPCHK(hipMemcpy(out.data(), src, out.size(), hipMemcpyDeviceToHost));
    return VR_OK;
}

static vr_status get_tree_common(BrickSet &b, Stream2 &s, int brick, uint8_t *dst, int64_t cap)
{
    vr_status rc = sync_ctrl(b);
    if (rc != VR_OK) return rc;
    int64_t bytes = ((int64_t)b.hostCtrl[brick].numActive + 3) / 4;
    if (!dst || cap < bytes) return VR_ERR_INVALID;
    const uint8_t *src = nullptr;
    rc = contiguous_stream(b, s, brick, &src);
    if (rc != VR_OK) return rc;
    if (b.hostCtrl[brick].emitOverflow) return VR_ERR_STATE;
    HIPCHK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return VR_OK;
}

vr_status vr_brickset_get_tree(vr_brickset *h, int32_t brick, uint8_t *dst, int64_t cap)
{
    if (!h || brick < 0 || brick >= h->s.B) return VR_ERR_INVALID;
    return get_tree_common(h->s, h->s.mid, brick, dst, cap);
}

vr_status vr_brickset_get_distance_map(vr_brickset *h, int32_t brick, uint8_t *dst, int32_t cap)
{
    if (!h || !dst || brick < 0 || brick >= h->s.B) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    vr_status rc = sync_ctrl(b);
    if (rc != VR_OK) return rc;
    if (cap < b.maxDepth + 1) return VR_ERR_INVALID;
    memcpy(dst, b.hostCtrl[brick].distanceMap, (size_t)b.maxDepth + 1);
    return VR_OK;
}

vr_status vr_brickset_get_tree_range(vr_brickset *h, int32_t brick, uint8_t *dst, int64_t cap)
{
    if (!h || brick < 0 || brick >= h->s.B) return VR_ERR_INVALID;
    if (h->s.variant != VR_VARIANT_MIDRANGE || (h->s.foreign && !h->s.foreignRange)) return VR_ERR_STATE;
    return get_tree_common(h->s, h->s.rng, brick, dst, cap);
}

vr_status vr_brickset_get_distance_map_range(vr_brickset *h, int32_t brick, uint8_t *dst, int32_t cap)
{
    if (!h || !dst || brick < 0 || brick >= h->s.B) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    if (b.variant != VR_VARIANT_MIDRANGE || (b.foreign && !b.foreignRange)) return VR_ERR_STATE;
    vr_status rc = sync_ctrl(b);
    if (rc != VR_OK) return rc;
    if (cap < b.maxDepth + 1) return VR_ERR_INVALID;
    Ctrl c;
    HIPCHK(hipMemcpy(&c, b.rng.ctrl + brick, sizeof(Ctrl), hipMemcpyDeviceToHost));
    memcpy(dst, c.distanceMap, (size_t)b.maxDepth + 1);
    return VR_OK;
}

// M.cpp:1095-1128 convertToByteArray.  A byte-shuffle of two host-visible streams:
// done on the host from the bytes the GPU encoder produced (format conversion, not
// part of the compute path).
vr_status vr_brickset_get_packed4(vr_brickset *h, int32_t brick, uint8_t *dst, int64_t cap, int64_t *length)
{
    if (!h || !length || brick < 0 || brick >= h->s.B) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    if (b.variant != VR_VARIANT_MIDRANGE || (b.foreign && !b.foreignRange)) return VR_ERR_STATE;
    vr_status rc = sync_ctrl(b);
    if (rc != VR_OK) return rc;
    const int64_t n = (int64_t)b.hostCtrl[brick].numActive;
    int64_t v = (int64_t)ceil((double)n / 2.0);
    v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; v++;
    *length = v;
    if (!dst) return VR_OK;
    if (cap < v) return VR_ERR_INVALID;
    const int64_t bytes = (n + 3) / 4;
    std::vector<uint8_t> m((size_t)bytes), r((size_t)bytes);
    const uint8_t *baseM = nullptr, *baseR = nullptr;
    rc = contiguous_stream(b, b.mid, brick, &baseM);
    if (rc == VR_OK) rc = contiguous_stream(b, b.rng, brick, &baseR);
    if (rc != VR_OK) return rc;
    HIPCHK(hipMemcpy(m.data(), baseM, (size_t)bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(r.data(), baseR, (size_t)bytes, hipMemcpyDeviceToHost));
    memset(dst, 0, (size_t)v);
    int64_t o = 0;
    for (int64_t i = 0; i < n; i += 2) {
        int first = cget(m.data(), i), second = cget(r.data(), i), third = 0, fourth = 0;
        if (i + 1 < n) { third = cget(m.data(), i + 1); fourth = cget(r.data(), i + 1); }
        dst[o++] = (uint8_t)((first << 6) | (second << 4) | (third << 2) | fourth);
    }
    return VR_OK;
}

// The one route for "foreign set, cut above Ds": the scalar of every depth-Ds subtree's ancestor at the brick's cut,
// into dst (B * nIdx).  cuts: per brick (only those in [0, Ds) are filled), or null: every brick at `cut`.  Bricks
// installed by vr_brickset_set_trees: from the heap their install wrote, on the stream -- a uniform cut run by run; a
// per-brick decode in one launch over the nTop bricks its uploaded image lists first (imageDev: LodPlan::image).  The
// others: from the stream bytes kept at set_tree/open time, by blocking copies, after sync_ctrl (numActive, distanceMap)
static vr_status foreign_cut_values(BrickSet &b, uint8_t *dst, const int32_t *cuts, int cut, const int32_t *imageDev, int nTop,
                                    hipStream_t st)
{
    const auto host = [&](int br) { const int c = cuts ? cuts[br] : cut; return c >= 0 && c < b.Ds && !top_indexed(b, br); };
    if (imageDev && cut_from_top_launch(&b, imageDev + b.B, imageDev, 0, nTop, 0, dst, st) != 0) return VR_ERR_NO_DEVICE;
    for (int br = 0; !imageDev && br < b.B;) {
        if (!top_indexed(b, br)) { ++br; continue; }
        int e = br;
        while (e < b.B && top_indexed(b, e)) ++e;
        if (cut_from_top_launch(&b, nullptr, nullptr, br, e - br, cut, dst, st) != 0) return VR_ERR_NO_DEVICE;
        br = e;
    }
    bool hostFill = false;
    for (int br = 0; br < b.B; ++br) hostFill = hostFill || host(br);
    const vr_status rc = hostFill ? sync_ctrl(b) : VR_OK;
    if (rc != VR_OK) return rc;
    std::vector<uint8_t> vals;
    for (int br = 0; br < b.B; ++br) {
        if (!host(br)) continue;
        vals.assign((size_t)b.nIdx, 0);
        if (br < (int)b.hostTree.size() && !b.hostTree[br].empty() &&
            cut_values_from_stream(b.D, b.Ds, b.K, b.nIdx, b.hostTree[br].data(), (int64_t)b.hostCtrl[br].numActive,
                                   b.hostCtrl[br].distanceMap, cuts ? cuts[br] : cut, vals) != 0)
            return VR_ERR_FORMAT;
        HIPCHK(hipMemcpy(dst + (size_t)br * b.nIdx, vals.data(), vals.size(), hipMemcpyHostToDevice));
    }
    return VR_OK;
}

// rangeStream: a MidRangeTree's half-range stream (vr_brickset_decode_range)
static vr_status decode_common(vr_brickset *h, int32_t cut_depth, uint8_t *out, void *stream, bool rangeStream)
{
    if (!h || !out) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    if (!b.built) return VR_ERR_STATE;
    if (rangeStream && b.variant != VR_VARIANT_MIDRANGE) return VR_ERR_STATE;
    if (rangeStream && b.foreign) return VR_ERR_UNSUPPORTED;   // an opened file carries no BFS codes to seed the index scalars from
    if (cut_depth > b.maxDepth) return VR_ERR_INVALID;
    const int cut = cut_depth < 0 ? b.maxDepth : cut_depth;
    const hipStream_t st = (hipStream_t)stream;
    const DecodePlan plan = make_decode_plan(decode_inputs(b, rangeStream), cut);
    if (plan.storesVectors && misaligned16(out)) return VR_ERR_INVALID;
    vr_status rc = ensure_decode_scratch(b, plan.needs, b.idxValCut, b.decTables, b.rankVals, st);
    if (rc != VR_OK) return rangeStream ? VR_ERR_NO_DEVICE : rc;      // (the range decode never named out-of-memory)
    if (plan.cutValues == CutSource::CALLER) rc = foreign_cut_values(b, b.idxValCut, nullptr, cut, nullptr, 0, st);
    if (rc != VR_OK) return rc;
    if (decode_launch(&b, plan, out, st) != 0) return VR_ERR_NO_DEVICE;
    b.decodeTimingPending = true;
    b.lastStream = stream;
    return VR_OK;
}

vr_status vr_brickset_decode(vr_brickset *h, int32_t cut_depth, uint8_t *out, void *stream)
{
    return decode_common(h, cut_depth, out, stream, false);
}

vr_status vr_brickset_decode_range(vr_brickset *h, int32_t cut_depth, uint8_t *out, void *stream)
{
    return decode_common(h, cut_depth, out, stream, true);
}

// the launch of the two per-brick decodes (cuts checked); the caller's buffer is out or pool->pool
static vr_status lod_decode(BrickSet &b, const int32_t *cuts, uint8_t *out, const PoolDest *pool, void *stream)
{
    const hipStream_t st = (hipStream_t)stream;
    uint8_t *dst = pool ? pool->pool : out;
    std::vector<uint8_t> top;
    for (int br = 0; b.foreign && br < b.B; ++br) top.push_back(top_indexed(b, br));
    const LodPlan plan = make_lod_plan(decode_inputs(b, false), cuts, b.foreign ? top.data() : nullptr, pool ? pool->off : nullptr,
                                       pool ? pool->shift : nullptr, pool && pool->tabDev ? pool->cells : 0);
    if (plan.storesVectors && misaligned16(dst)) return VR_ERR_INVALID;
    if (plan.nothing) return VR_OK;
    LodSlot *s = nullptr;
    vr_status rc = ensure_lod_slot(b, plan, st, s);
    if (rc != VR_OK) return rc;
    // from here on the slot is in use: decode_lod_launch ends with its event, and so does a failure in front of it
    if (lod_stage(&b, plan, *s, pool ? pool->tab : nullptr, pool ? pool->tabDev : nullptr, st) != 0) rc = VR_ERR_NO_DEVICE;
    if (rc == VR_OK && plan.cutValues == CutSource::CALLER) rc = foreign_cut_values(b, s->idxValCut, cuts, 0, s->dev, plan.nTop, st);
    if (rc != VR_OK) { hipEventRecord(s->done, st); s->pending = true; return rc; }
    if (decode_lod_launch(&b, plan, *s, dst, st) != 0) return VR_ERR_NO_DEVICE;
    b.decodeTimingPending = true;
    b.lastStream = stream;
    return VR_OK;
}

vr_status vr_brickset_decode_lod(vr_brickset *h, const int32_t *cuts, uint8_t *out, void *stream)
{
    if (!h || !cuts || !out) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    if (!b.built) return VR_ERR_STATE;
    for (int br = 0; br < b.B; ++br) if (cuts[br] < -1 || cuts[br] > b.maxDepth) return VR_ERR_INVALID;
    return lod_decode(b, cuts, out, nullptr, stream);
}

vr_status vr_lod_pool_layout(const int64_t brick_dims[3], int32_t num_bricks, const int64_t *brick_ijk, const int64_t grid[3],
                             const int32_t *cuts, int32_t orig_tree_depth, int32_t max_tree_depth, vr_pool_entry *table_out,
                             int64_t *pool_bytes)
{
    if (!brick_dims || !brick_ijk || !grid || !cuts || !pool_bytes || num_bricks <= 0) return VR_ERR_INVALID;
    std::vector<int64_t> off((size_t)num_bricks);
    std::vector<uint8_t> sh((size_t)num_bricks * 3);
    return (vr_status)pool_layout(brick_dims, num_bricks, brick_ijk, grid, cuts, orig_tree_depth, max_tree_depth, off.data(),
                                  sh.data(), table_out, pool_bytes);
}

vr_status vr_brickset_decode_lod_pool(vr_brickset *h, const int32_t *cuts, const int64_t *ijk, const int64_t grid[3],
                                      uint8_t *pool, int64_t pool_bytes, vr_pool_entry *table_dev, void *stream)
{
    if (!h || !cuts || !ijk || !grid || !pool) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    if (!b.built) return VR_ERR_STATE;
    const int64_t bd[3] = {b.g.X, b.g.Y, b.g.Z};
    for (int k = 0; k < 3; ++k) if ((bd[k] & (bd[k] - 1)) != 0) return VR_ERR_UNSUPPORTED;
    for (int k = 0; k < 3; ++k) if (grid[k] <= 0) return VR_ERR_INVALID;
    const int64_t cells = grid[0] * grid[1] * grid[2];
    std::vector<int64_t> off((size_t)b.B);
    std::vector<uint8_t> sh((size_t)b.B * 3);
    std::vector<vr_pool_entry> tab((size_t)cells);
    int64_t total = 0;
    const vr_status st = (vr_status)pool_layout(bd, b.B, ijk, grid, cuts, b.D, b.maxDepth, off.data(), sh.data(), tab.data(), &total);
    if (st != VR_OK) return st;
    if (pool_bytes < total) return VR_ERR_INVALID;
    PoolDest d;
    d.pool = pool; d.off = off.data(); d.shift = sh.data(); d.tab = tab.data(); d.tabDev = table_dev; d.cells = cells;
    return lod_decode(b, cuts, nullptr, &d, stream);
}

// The frame of vr_raycast is view_basis (raymarch.h).  Every ray of the frame is dir = f + nx tanX s + ny tanY u,
// |nx|, |ny| < 1; its ray parameter is the view depth d . f (d = point - pos), and its march starts at depth >= z_near.
vr_status vr_lod_select(const vr_camera *cam, const vr_render_params *P, int32_t num_bricks, const int64_t brick_dims[3],
                        const int64_t *brick_ijk, const int64_t grid[3], int32_t orig_tree_depth, int32_t max_tree_depth,
                        float pixel_tolerance, int32_t *cuts_out)
{
    if (!cam || !P || !brick_dims || !brick_ijk || !grid || !cuts_out || num_bricks <= 0) return VR_ERR_INVALID;
    if (!(pixel_tolerance > 0.0f) || P->width <= 0 || P->height <= 0) return VR_ERR_INVALID;
    if (orig_tree_depth < 0 || max_tree_depth < orig_tree_depth) return VR_ERR_INVALID;
    for (int k = 0; k < 3; ++k) if (brick_dims[k] <= 0 || grid[k] <= 0) return VR_ERR_INVALID;
    double G[3], vs[3], vmax = 0.0;
    for (int k = 0; k < 3; ++k) {
        G[k] = P->global_dims[k] > 0 ? (double)P->global_dims[k] : (double)(grid[k] * brick_dims[k]);
        vs[k] = 1.0 / G[k];
        vmax = std::max(vmax, vs[k]);
    }
    // the reach beyond a brick's voxels of the samples and taps that read them: one voxel (a trilinear tap), two in
    // shaded mode; in iso-surface mode also the gradient's 0.01 offset and one step (the second fetch and the bisection, whose points
    // may lie outside the cube and read its clamped edge)
    double grow[3], stepMax = 0.0;
    for (int k = 0; k < 3; ++k) stepMax = std::max(stepMax, (double)fabsf(P->step_size[k]));
    for (int k = 0; k < 3; ++k) grow[k] = vs[k] + (P->mode == VR_RENDER_ISOSURFACE ? 0.01 + stepMax : 0.0);
    if (P->mode == VR_RENDER_SHADED)    // the lattice gradient's taps reach one voxel beyond the trilinear taps
        for (int k = 0; k < 3; ++k) grow[k] = 2.0 * vs[k];
    const ViewBasis vb = view_basis(cam, P->width, P->height);
    const float *f = vb.f, *sv = vb.s, *u = vb.u;
    const double tanY = vb.tanY, tanX = vb.tanX;
    const bool basis = (sv[0] != 0.0f || sv[1] != 0.0f || sv[2] != 0.0f);
    // a ray marches at most max_samples + 1 steps past its entry point (at depth <= z_far)
    const double zNear = cam->z_near, zFar = (double)cam->z_far + ((double)std::max(P->max_samples, 0) + 1.0) * stepMax;
    const double eps = 1e-6;     // float rounding of the ray positions
    const double focal = (double)P->height / 2.0 / tanY;
    for (int i = 0; i < num_bricks; ++i) {
        double lo[3], hi[3];        // the grown box, in the world space of vr_raycast's cube [-0.5, 0.5]^3
        for (int k = 0; k < 3; ++k) {
            lo[k] = (double)(brick_ijk[3 * i + k] * brick_dims[k]) * vs[k] - grow[k] - 0.5;
            hi[k] = (double)((brick_ijk[3 * i + k] + 1) * brick_dims[k]) * vs[k] + grow[k] - 0.5;
        }
        bool culled = false;
        for (int k = 0; k < 3; ++k)       // [box_min, box_max) in texture space
            if (hi[k] + 0.5 < (double)P->box_min[k] || lo[k] + 0.5 >= (double)P->box_max[k]) culled = true;
        // frustum: all eight corners outside one plane (depth below z_near or above the far bound, |x| > tanX depth,
        // |y| > tanY depth)
        int outN = 0, outF = 0, outL = 0, outR = 0, outB = 0, outT = 0;
        for (int c = 0; c < 8; ++c) {
            const double p[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
            double d[3], z = 0.0, x = 0.0, y = 0.0;
            for (int k = 0; k < 3; ++k) d[k] = p[k] - (double)cam->pos[k];
            for (int k = 0; k < 3; ++k) { z += d[k] * f[k]; x += d[k] * sv[k]; y += d[k] * u[k]; }
            const double tol = eps * (1.0 + fabs(z));
            outN += z < zNear - tol;
            outF += z > zFar + tol;
            outR += x > tanX * z + tol; outL += -x > tanX * z + tol;
            outT += y > tanY * z + tol; outB += -y > tanY * z + tol;
        }
        if (outN == 8 || outF == 8) culled = true;
        if (basis && (outR == 8 || outL == 8 || outT == 8 || outB == 8)) culled = true;
        if (culled) { cuts_out[i] = -1; continue; }
        double q = 0.0;               // distance from the camera to the grown box
        for (int k = 0; k < 3; ++k) {
            const double e = std::max(std::max(lo[k] - (double)cam->pos[k], 0.0), (double)cam->pos[k] - hi[k]);
            q += e * e;
        }
        const double s = focal * vmax / std::max(sqrt(q), zNear);
        int k = 0;
        if (s < (double)pixel_tolerance)
            k = (int)std::min((double)orig_tree_depth, floor(3.0 * log2((double)pixel_tolerance / s)));
        cuts_out[i] = k == 0 ? max_tree_depth : orig_tree_depth - k;
    }
    return VR_OK;
}

// ---- an install, in the order of a build: plan (host_plan.h make_install_plan: every refusal), the host pass over each
// stream or table (VR_ERR_FORMAT), ensure every buffer the plan's `needs` names (VR_ERR_OOM), and only then the first
// write to the set or to device memory.  A return up to there leaves the set as it was.
static InstallInputs install_inputs(const BrickSet &b, InstallEngine engine, int32_t count, const int32_t *bricks, const vr_tree_desc *descs)
{
    InstallInputs in{};
    in.D = b.D; in.Ds = b.Ds; in.K = b.K; in.B = b.B; in.maxDepth = b.maxDepth; in.variant = b.variant;
    in.nIdx = b.nIdx; in.treeCap = b.treeCap;
    in.idx64 = b.idx64; in.built = b.built; in.foreign = b.foreign;
    in.engine = engine; in.count = count; in.bricks = bricks; in.descs = descs;
    return in;
}

// a new idxTop is zero-filled: entry 0 of a heap, and the heap of a brick never installed, are never written otherwise
static vr_status ensure_install_buffers(BrickSet &b, const InstallPlan &p)
{
    const size_t B = (size_t)b.B, nIdx = (size_t)b.nIdx;
    const InstallNeeds &n = p.needs;
    if (n.idxTop && !b.idxTop) {
        if (!ensure_dev(b.idxTop, B * nIdx * 2)) { (void)hipGetLastError(); return VR_ERR_OOM; }
        if (hipMemset(b.idxTop, 0, B * nIdx * 2) != hipSuccess) { hipFree(b.idxTop); b.idxTop = nullptr; return VR_ERR_NO_DEVICE; }
    }
    if ((n.instOff && !ensure_dev(b.instOff, B * (size_t)p.nBlk * sizeof(uint32_t))) || (n.instFlag && !ensure_dev(b.instFlag, B * sizeof(int32_t))) ||
        (n.instList && !ensure_dev(b.instList, B * sizeof(int32_t))) || (n.fineIdx && !ensure_dev(b.fineIdx, B * nIdx * 16)) ||
        (n.idxVal3 && !ensure_dev(b.idxVal3, B * nIdx * 8)) || (n.idxBase && !ensure_dev(b.idxBase, B * (size_t)b.nEmitBlk * sizeof(unsigned long long)))) {
        (void)hipGetLastError();
        return VR_ERR_OOM;
    }
    return VR_OK;
}

// The whole set to "never installed": host controls zero, every index offset dead, index scalars and side-cars zero
// (k_index_reset over all bricks, on st).  The device's controls follow with the caller's upload of hostCtrl, whole.
static vr_status never_installed(BrickSet &b, hipStream_t st)
{
    for (auto &c : b.hostCtrl) memset(&c, 0, sizeof(Ctrl));
    b.fineHas.assign((size_t)b.B, 1);       // (every offset is dead: no counts are read)
    return index_reset_launch(&b, nullptr, b.B, nullptr, false, st) == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

// the one place a set becomes one of installed streams
static void mark_installed(BrickSet &b)
{
    b.built = true;
    b.hostCtrlValid = true;
    b.foreign = true;
    b.gapped = false;          // an installed stream is the contiguous one; its index points into it
    if (b.fineHas.size() != (size_t)b.B) b.fineHas.assign((size_t)b.B, 0);
    if (b.hostTree.size() != (size_t)b.B) b.hostTree.assign((size_t)b.B, std::vector<uint8_t>());
}

// the buffers, then the first writes of an install: a fresh set starts out never installed, any other brings its host controls up to date
static vr_status begin_install(BrickSet &b, const InstallPlan &p, hipStream_t st)
{
    vr_status rc = ensure_install_buffers(b, p);
    if (rc == VR_OK) rc = p.firstInstall ? never_installed(b, st) : sync_ctrl(b);
    if (rc == VR_OK) mark_installed(b);
    return rc;
}

// a brick's new stream on the host: its control block; no host bytes and no fine side-car until the engine says so
static void record_brick(BrickSet &b, size_t br, const vr_tree_desc &d)
{
    Ctrl &c = b.hostCtrl[br];
    memset(&c, 0, sizeof(Ctrl));
    c.numActive = (unsigned long long)d.num_active;
    memcpy(c.distanceMap, d.distance_map, (size_t)b.maxDepth + 1);
    std::vector<uint8_t>().swap(b.hostTree[br]);
    b.fineHas[br] = 0;
}

// the host-parsed engine: blocking copies; the stream's bytes are kept for cuts above depth Ds
vr_status vr_brickset_set_tree(vr_brickset *h, int32_t brick, const uint8_t *tree, int64_t tree_bytes,
                               int64_t num_active, const uint8_t *dmap, int32_t map_len)
{
    if (!h) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    const vr_tree_desc d = {tree, tree_bytes, num_active, dmap, map_len, nullptr, nullptr};
    const InstallPlan p = make_install_plan(install_inputs(b, InstallEngine::HOST_PARSE, 1, &brick, &d));
    if (p.status != VR_OK) return (vr_status)p.status;
    const InstallBrick &pb = p.brick[0];
    std::vector<uint32_t> offs;
    std::vector<uint8_t> vals, fine, val3;
    if (build_index_from_stream(b.D, b.Ds, b.K, b.nIdx, tree, num_active, dmap, offs, vals, fine, val3) != 0) return VR_ERR_FORMAT;
    const vr_status rc = begin_install(b, p, nullptr);      // (the null stream: in front of the blocking copies)
    if (rc != VR_OK) return rc;
    const size_t br = (size_t)brick, nIdx = (size_t)b.nIdx;
    record_brick(b, br, d);
    fine_has_changed(b);
    if (p.firstInstall) HIPCHK(hipMemcpy(b.mid.ctrl, b.hostCtrl.data(), (size_t)b.B * sizeof(Ctrl), hipMemcpyHostToDevice));
    else HIPCHK(hipMemcpy(b.mid.ctrl + br, &b.hostCtrl[br], sizeof(Ctrl), hipMemcpyHostToDevice));
    uint8_t *slot = b.mid.tree + br * (size_t)b.treeCap;
    HIPCHK(hipMemset(slot, 0, (size_t)b.treeCap));
    HIPCHK(hipMemcpy(slot, tree, (size_t)pb.need, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b.idxOff + br * nIdx, offs.data(), offs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b.idxVal + br * nIdx, vals.data(), vals.size(), hipMemcpyHostToDevice));
    if (p.needs.idxBase) HIPCHK(hipMemset(b.idxBase, 0, (size_t)b.B * b.nEmitBlk * sizeof(unsigned long long)));
    if (install_fine_has(pb, false)) {
        HIPCHK(hipMemcpy(b.fineIdx + br * nIdx * 16, fine.data(), fine.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.idxVal3 + br * nIdx * 8, val3.data(), val3.size(), hipMemcpyHostToDevice));
        b.fineHas[br] = 1;
        fine_has_changed(b);
    }
    b.hostTree[br].assign(tree, tree + pb.need);
    return VR_OK;
}

// vrhip.h "compressed brick-set archives": the device engine.  The copies and the kernels of kd_index.hip go to
// `stream`, and one synchronisation reads the grammar flags.  No host bytes are kept: cuts above depth Ds come from idxTop.
vr_status vr_brickset_set_trees(vr_brickset *h, int32_t count, const int32_t *bricks, const vr_tree_desc *descs, void *stream)
{
    if (!h) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    const InstallPlan p = make_install_plan(install_inputs(b, InstallEngine::DEVICE_INDEX, count, bricks, descs));
    if (p.status != VR_OK) return (vr_status)p.status;
    const size_t nBlk = (size_t)p.nBlk, B = (size_t)b.B;
    std::vector<std::vector<uint32_t>> madeOff((size_t)count);
    std::vector<std::vector<uint8_t>> madeTop((size_t)count);
    std::atomic<int> bad(0);
    parallel_for(count, [&](int i) {
        const vr_tree_desc &d = descs[i];
        if (p.brick[(size_t)i].pass == HostPass::TABLE_CHECK) { if (!block_table_ok(b.D, d.num_active, d.block_off)) bad = 1; return; }
        madeOff[(size_t)i].resize(nBlk);
        madeTop[(size_t)i].resize(2 * nBlk);
        if (block_table_from_stream(b.D, d.tree, d.num_active, d.distance_map, madeOff[(size_t)i].data(), madeTop[(size_t)i].data()) != 0) bad = 1;
    });
    if (bad) return VR_ERR_FORMAT;
    hipStream_t st = (hipStream_t)stream;
    const vr_status rc = begin_install(b, p, st);
    if (rc != VR_OK) return rc;
    b.lastStream = stream;
    for (int i = 0; i < count; ++i) {
        const vr_tree_desc &d = descs[i];
        const InstallBrick &pb = p.brick[(size_t)i];
        const size_t br = (size_t)bricks[i];
        record_brick(b, br, d);
        uint8_t *slot = b.mid.tree + br * (size_t)b.treeCap;
        HIPCHK(hipMemcpyAsync(slot, d.tree, (size_t)pb.need, hipMemcpyHostToDevice, st));
        if (pb.tail > 0) HIPCHK(hipMemsetAsync(slot + pb.need, 0, (size_t)pb.tail, st));
        HIPCHK(hipMemcpyAsync(b.instOff + br * nBlk, d.block_off ? d.block_off : madeOff[(size_t)i].data(), nBlk * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        // (the table's heap IS the top of the brick's: the same layout, depths 0 .. Dc)
        HIPCHK(hipMemcpyAsync(b.idxTop + br * (size_t)b.nIdx * 2, d.top_val ? d.top_val : madeTop[(size_t)i].data(), 2 * nBlk, hipMemcpyHostToDevice, st));
    }
    fine_has_changed(b);
    HIPCHK(hipMemcpyAsync(b.mid.ctrl, b.hostCtrl.data(), B * sizeof(Ctrl), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b.instList, bricks, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b.instFlag, 0, (size_t)count * sizeof(int32_t), st));
    if (index_reset_launch(&b, b.instList, count, nullptr, false, st) != 0) return VR_ERR_NO_DEVICE;
    if (index_from_stream_launch(&b, b.instList, count, b.instFlag, st) != 0) return VR_ERR_NO_DEVICE;
    if (index_reset_launch(&b, b.instList, count, b.instFlag, true, st) != 0) return VR_ERR_NO_DEVICE;
    std::vector<int32_t> flags((size_t)count, 0);
    HIPCHK(hipMemcpyAsync(flags.data(), b.instFlag, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const bool failed = std::find_if(flags.begin(), flags.end(), [](int32_t f) { return f != 0; }) != flags.end();
    for (int i = 0; i < count; ++i) {
        const size_t br = (size_t)bricks[i];
        b.fineHas[br] = install_fine_has(p.brick[(size_t)i], failed);
        if (failed) memset(&b.hostCtrl[br], 0, sizeof(Ctrl));
    }
    fine_has_changed(b);
    if (failed) {       // every brick named in the call is left never installed
        if (index_reset_launch(&b, b.instList, count, nullptr, true, st) != 0) return VR_ERR_NO_DEVICE;
        HIPCHK(hipStreamSynchronize(st));
        return VR_ERR_FORMAT;
    }
    return VR_OK;
}

static vr_status archive_matches(const BrickSet &b, const ArchiveGeom &g)
{
    const bool same = g.variant == b.variant && g.numBricks == b.B && g.D == b.D && g.maxDepth == b.maxDepth &&
                      g.dims[0] == b.g.X && g.dims[1] == b.g.Y && g.dims[2] == b.g.Z;
    return same ? VR_OK : VR_ERR_FORMAT;
}

static vr_status install_archive(BrickSet &b, vr_brickset *h, const void *blob, const ArchiveGeom &g,
                                 const std::vector<ArchiveEntry> &dir, void *stream)
{
    std::vector<int32_t> bricks;
    std::vector<vr_tree_desc> descs;
    for (int br = 0; br < g.numBricks; ++br) {
        const ArchiveEntry &e = dir[(size_t)br];
        if (e.offset == 0) continue;
        const ArchiveRecord r = archive_record(blob, g, e);
        bricks.push_back(br);
        descs.push_back(vr_tree_desc{r.tree, e.treeBytes, e.numActive, r.dmap, b.maxDepth + 1, r.blockOff, r.topVal});
    }
    if (bricks.empty()) return VR_OK;
    return vr_brickset_set_trees(h, (int32_t)bricks.size(), bricks.data(), descs.data(), stream);
}

vr_status vr_brickset_load_set_memory(vr_brickset *h, const void *blob, int64_t bytes, void *stream)
{
    if (!h || !blob || bytes <= 0 || misaligned16(blob)) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    if (b.variant == VR_VARIANT_MIDRANGE || b.idx64) return VR_ERR_UNSUPPORTED;
    if (b.built && !b.foreign) return VR_ERR_STATE;
    ArchiveGeom g;
    std::vector<ArchiveEntry> dir;
    if (archive_parse(blob, bytes, g, dir) != 0) return VR_ERR_FORMAT;
    vr_status rc = archive_matches(b, g);
    if (rc != VR_OK) return rc;
    return install_archive(b, h, blob, g, dir, stream);
}

// a whole file in one pinned buffer (the caller frees it with hipHostFree)
static vr_status read_archive_file(const char *path, void **blob, int64_t *bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) return VR_ERR_IO;
    fseek(f, 0, SEEK_END);
    const int64_t n = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (n < VR_ARCHIVE_HEADER_BYTES) { fclose(f); return n < 0 ? VR_ERR_IO : VR_ERR_FORMAT; }
    void *p = nullptr;
    if (hipHostMalloc(&p, (size_t)n, hipHostMallocDefault) != hipSuccess) { fclose(f); return VR_ERR_OOM; }
    const bool ok = fread(p, 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    if (!ok) { hipHostFree(p); return VR_ERR_IO; }
    *blob = p; *bytes = n;
    return VR_OK;
}

vr_status vr_brickset_load_set(vr_brickset *h, const char *path, void *stream)
{
    if (!h || !path) return VR_ERR_INVALID;
    void *blob = nullptr;
    int64_t bytes = 0;
    vr_status rc = read_archive_file(path, &blob, &bytes);
    if (rc != VR_OK) return rc;
    rc = vr_brickset_load_set_memory(h, blob, bytes, stream);     // (synchronises `stream`: the buffer is done with)
    hipHostFree(blob);
    return rc;
}

vr_status vr_brickset_open_set(vr_brickset **out, const char *path, void *stream)
{
    if (!out || !path) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    void *blob = nullptr;
    int64_t bytes = 0;
    vr_status rc = read_archive_file(path, &blob, &bytes);
    if (rc != VR_OK) return rc;
    ArchiveGeom g;
    std::vector<ArchiveEntry> dir;
    vr_brickset *h = nullptr;
    if (archive_parse(blob, bytes, g, dir) != 0) rc = VR_ERR_FORMAT;
    if (rc == VR_OK && (g.variant < 0 || g.variant > 2)) rc = VR_ERR_FORMAT;
    if (rc == VR_OK && g.variant == VR_VARIANT_MIDRANGE) rc = VR_ERR_UNSUPPORTED;
    if (rc == VR_OK) rc = vr_brickset_create(&h, g.numBricks, g.dims, 6, 5, g.variant);   // (vr_brickset_open's defaults)
    if (rc == VR_OK) rc = archive_matches(h->s, g);
    if (rc == VR_OK) rc = install_archive(h->s, h, blob, g, dir, stream);
    hipHostFree(blob);
    if (rc != VR_OK) { vr_brickset_destroy(h); return rc; }
    *out = h;
    return VR_OK;
}

vr_status vr_brickset_save_set(vr_brickset *h, const char *path)
{
    if (!h || !path) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    if (b.variant == VR_VARIANT_MIDRANGE || b.idx64) return VR_ERR_UNSUPPORTED;
    vr_status rc = sync_ctrl(b);
    if (rc != VR_OK) return rc;
    const int Dc = block_depth(b.D);
    std::vector<std::vector<uint8_t>> trees((size_t)b.B);
    std::vector<ArchiveBrick> bricks((size_t)b.B);
    for (int br = 0; br < b.B; ++br) {
        const Ctrl &c = b.hostCtrl[(size_t)br];
        if (c.numActive == 0ull) continue;
        if (c.numActive >= (1ull << 32)) return VR_ERR_UNSUPPORTED;
        rc = download_stream(b, b.mid, br, trees[(size_t)br]);
        if (rc != VR_OK) return rc;
        if (b.hostCtrl[(size_t)br].emitOverflow) return VR_ERR_STATE;
    }
    std::atomic<int> bad(0);
    parallel_for(b.B, [&](int br) {
        const Ctrl &c = b.hostCtrl[(size_t)br];
        if (trees[(size_t)br].empty()) return;
        ArchiveBrick &k = bricks[(size_t)br];
        k.numActive = (int64_t)c.numActive; k.dmap = c.distanceMap; k.tree = trees[(size_t)br].data();
        k.blockOff.resize((size_t)1 << Dc);
        k.topVal.resize((size_t)2 << Dc);
        if (block_table_from_stream(b.D, k.tree, k.numActive, k.dmap, k.blockOff.data(), k.topVal.data()) != 0) bad = 1;
    });
    if (bad) return VR_ERR_STATE;
    FILE *f = fopen(path, "wb");
    if (!f) return VR_ERR_IO;
    const ArchiveGeom g = {b.variant, {b.g.X, b.g.Y, b.g.Z}, b.B, b.D, b.maxDepth};
    const bool ok = archive_write(f, g, bricks);
    return (fclose(f) == 0 && ok) ? VR_OK : VR_ERR_IO;
}

// File layout of VolumeKdtree::save (R.cpp:535-544).
vr_status vr_brickset_save(vr_brickset *h, int32_t brick, const char *path)
{
    if (!h || !path || brick < 0 || brick >= h->s.B) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    vr_status rc = sync_ctrl(b);
    if (rc != VR_OK) return rc;                       // "ERROR! No tree to save." R.cpp:526-530
    const Ctrl &c = b.hostCtrl[brick];
    const int64_t bytes = ((int64_t)c.numActive + 3) / 4;
    if (bytes == 0) return VR_ERR_STATE;
    std::vector<uint8_t> tree, treeR;
    rc = download_stream(b, b.mid, brick, tree);
    if (rc != VR_OK) return rc;
    // MidRangeTree::save (M.cpp:753-785): same header, then distanceMap, distanceMap_range, tree, tree_range
    const bool mrFile = b.variant == VR_VARIANT_MIDRANGE;
    Ctrl cr;
    if (mrFile) {
        if (b.foreign && !b.foreignRange) return VR_ERR_STATE;
        rc = download_stream(b, b.rng, brick, treeR);     // (as many tokens as the mid stream's)
        if (rc != VR_OK) return rc;
        HIPCHK(hipMemcpy(&cr, b.rng.ctrl + brick, sizeof(Ctrl), hipMemcpyDeviceToHost));
    }
    FILE *f = fopen(path, "wb");
    if (!f) return VR_ERR_IO;
    const Header hd = {{0, 0, 0}, {b.g.X, b.g.Y, b.g.Z}, b.maxDepth, b.D, b.g.X, b.g.Y, b.g.Z, (int64_t)c.numActive};
    const size_t mtd = (size_t)b.maxDepth;
    bool ok = write_header(f, hd) &&
              fwrite(c.distanceMap, 1, mtd + 1, f) == mtd + 1 &&
              (!mrFile || fwrite(cr.distanceMap, 1, mtd + 1, f) == mtd + 1) &&
              fwrite(tree.data(), 1, (size_t)bytes, f) == (size_t)bytes &&
              (!mrFile || fwrite(treeR.data(), 1, (size_t)bytes, f) == (size_t)bytes);
    fclose(f);
    return ok ? VR_OK : VR_ERR_IO;
}

// a MidRangeTree file's half-range stream, beside the mid stream vr_brickset_set_tree installed (a 1-brick set: open_file)
static vr_status install_range_stream(BrickSet &b, const uint8_t *tree, int64_t bytes, int64_t numActive, const uint8_t *dmap)
{
    if (!ensure_dev(b.rng.ctrl, (size_t)b.B * sizeof(Ctrl)) || !ensure_dev(b.rng.tree, (size_t)b.B * b.treeCap)) { (void)hipGetLastError(); return VR_ERR_OOM; }
    Ctrl cr;
    memset(&cr, 0, sizeof(Ctrl));
    cr.numActive = (unsigned long long)numActive;
    memcpy(cr.distanceMap, dmap, (size_t)b.maxDepth + 1);
    if (hipMemcpy(b.rng.ctrl, &cr, sizeof(Ctrl), hipMemcpyHostToDevice) != hipSuccess || hipMemset(b.rng.tree, 0, (size_t)b.treeCap) != hipSuccess ||
        hipMemcpy(b.rng.tree, tree, (size_t)bytes, hipMemcpyHostToDevice) != hipSuccess) return VR_ERR_NO_DEVICE;
    b.foreignRange = true;
    return VR_OK;
}

// VolumeKdtree::open (R.cpp:554-594) and, mr, MidRangeTree files (M.cpp:753-785).  A missing file is an error code here
// (the reference waits for Enter and calls exit(-1)).  The reference's own MidRangeTree reader (M.cpp:787-833) mis-sizes
// both streams by 4 bytes (it subtracts three of the four int64 header fields before halving), so the range stream it
// reads back is shifted; there is nothing to match there.  This reader returns exactly what save() wrote.
static vr_status open_file(vr_brickset **out, const char *path, bool mr)
{
    if (!out || !path) return VR_ERR_INVALID;
    FILE *f = fopen(path, "rb");
    if (!f) return VR_ERR_IO;
    fseek(f, 0, SEEK_END);
    const int64_t fileSize = ftell(f);
    fseek(f, 0, SEEK_SET);
    Header hd;
    if (!read_header(f, hd)) { fclose(f); return VR_ERR_FORMAT; }
    const int64_t mtd = hd.maxDepth, na = hd.numActive, need = (na + 3) / 4;
    // VolumeKdtree: whatever follows the map is the stream (numActiveNodes is authoritative); MidRangeTree: two maps,
    // then two streams of exactly the tokens' bytes
    const int64_t have = fileSize - (VR_HEADER_BYTES + (mr ? 2 : 1) * (mtd + 1));
    const int64_t T = mr ? have / 2 : have;
    if (mr ? (have < 0 || (have & 1) || T != need) : have < need) { fclose(f); return VR_ERR_FORMAT; }
    std::vector<uint8_t> body((size_t)(fileSize - VR_HEADER_BYTES));
    const bool ok = fread(body.data(), 1, body.size(), f) == body.size();
    const uint8_t *dmap = body.data(), *dmapR = dmap + (mtd + 1), *tree = dmap + (mr ? 2 : 1) * (mtd + 1), *treeR = tree + T;
    fclose(f);
    if (!ok) return VR_ERR_IO;
    const int64_t dims[3] = {hd.X, hd.Y, hd.Z};
    vr_brickset *h = nullptr;
    vr_status rc = vr_brickset_create(&h, 1, dims, 6, 5, mr ? VR_VARIANT_MIDRANGE : VR_VARIANT_RECOVER); // ctor defaults R.h:89-94
    if (rc != VR_OK) return rc;
    BrickSet &b = h->s;
    if (b.D != hd.origDepth || b.maxDepth != mtd) { vr_brickset_destroy(h); return VR_ERR_FORMAT; }
    rc = vr_brickset_set_tree(h, 0, tree, T, na, dmap, (int32_t)mtd + 1);
    if (rc == VR_OK && mr) rc = install_range_stream(b, treeR, T, na, dmapR);
    if (rc != VR_OK) { vr_brickset_destroy(h); return rc; }
    *out = h;
    return VR_OK;
}

vr_status vr_brickset_open(vr_brickset **out, const char *path) { return open_file(out, path, false); }

vr_status vr_brickset_open_variant(vr_brickset **out, const char *path, int32_t variant)
{
    if (variant != VR_VARIANT_RECOVER && variant != VR_VARIANT_GUARDED && variant != VR_VARIANT_MIDRANGE) return VR_ERR_INVALID;
    return open_file(out, path, variant == VR_VARIANT_MIDRANGE);
}

vr_status vr_measure_error(const uint8_t *dec, const uint8_t *orig, int64_t n, int32_t *max_error, double *mean_error,
                           void *stream)
{
    if (!dec || !orig || n <= 0) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    int *dMax = nullptr;
    unsigned long long *dSum = nullptr;
    HIPCHK(hipMalloc(&dMax, sizeof(int)));
    const hipError_t e2 = hipMalloc(&dSum, sizeof(unsigned long long));
    if (e2 != hipSuccess) { hipFree(dMax); return e2 == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_NO_DEVICE; }
    hipMemsetAsync(dMax, 0, sizeof(int), (hipStream_t)stream);
    hipMemsetAsync(dSum, 0, sizeof(unsigned long long), (hipStream_t)stream);
    int rc = measure_error_launch(dec, orig, n, dMax, dSum, (hipStream_t)stream);
    int hm = 0;
    unsigned long long hs = 0;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpy(&hm, dMax, sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&hs, dSum, sizeof(hs), hipMemcpyDeviceToHost);
    hipFree(dMax); hipFree(dSum);
    if (rc != 0 || e != hipSuccess) return VR_ERR_NO_DEVICE;
    if (max_error) *max_error = hm;
    if (mean_error) *mean_error = (double)hs / (double)n;
    return VR_OK;
}

vr_status vr_query_error(const uint8_t *dec, const uint8_t *orig, int64_t n, uint8_t *err, void *stream)
{
    if (!dec || !orig || !err || n <= 0) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return query_error_launch(dec, orig, n, err, (hipStream_t)stream) == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

// the reduction alone (error_table.hip): a device table of its own for the call
vr_status vr_measure_error_bricks(const uint8_t *dec, const uint8_t *ref, int32_t num_bricks, int64_t voxels_per_brick,
                                  vr_brick_error *out, void *stream)
{
    if (!dec || !ref || !out || num_bricks < 1 || voxels_per_brick < 1 || voxels_per_brick > 0xFFFFFFFFll) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    const size_t bytes = (size_t)num_bricks * sizeof(vr_brick_error);
    vr_brick_error *dTab = nullptr;
    HIPCHK(hipMalloc(&dTab, bytes));
    hipError_t e = hipMemsetAsync(dTab, 0, bytes, (hipStream_t)stream);
    int rc = 0;
    if (e == hipSuccess) rc = brick_error_launch(dec, ref, num_bricks, voxels_per_brick, dTab, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dTab, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream);
    const hipError_t es = hipStreamSynchronize((hipStream_t)stream);
    hipFree(dTab);
    return rc != 0 || e != hipSuccess || es != hipSuccess ? VR_ERR_NO_DEVICE : VR_OK;
}

// vrhip.h "error-bounded level of detail": per cut the set's uniform decode into the scratch, then the reduction into
// that cut's row of the set's device table
vr_status vr_brickset_error_table(vr_brickset *h, const uint8_t *ref, uint8_t *scratch, int32_t cut_lo, int32_t cut_hi,
                                  vr_brick_error *table, void *stream)
{
    if (!h || !ref || !scratch || !table) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    if (cut_lo < 0 || cut_hi > b.maxDepth || cut_lo > cut_hi) return VR_ERR_INVALID;
    if (!b.built) return VR_ERR_STATE;
    for (int c = cut_lo; c <= cut_hi; ++c)
        if (make_decode_plan(decode_inputs(b, false), c).storesVectors && misaligned16(scratch)) return VR_ERR_INVALID;
    const size_t row = (size_t)b.B * sizeof(vr_brick_error), bytes = row * (size_t)(cut_hi - cut_lo + 1);
    if (!b.errTable) HIPCHK(hipMalloc(&b.errTable, row * (size_t)(b.maxDepth + 1)));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(b.errTable, 0, bytes, st));
    for (int c = cut_lo; c <= cut_hi; ++c) {
        // a foreign set's cut values above the index level are written by a blocking copy from the host: the decode
        // of the cut before must have read its own first
        if (b.foreign && c < b.Ds) HIPCHK(hipStreamSynchronize(st));
        const vr_status rc = decode_common(h, c, scratch, stream, false);
        if (rc != VR_OK) { hipStreamSynchronize(st); return rc; }
        if (brick_error_launch(scratch, ref, b.B, b.g.voxels, b.errTable + (size_t)(c - cut_lo) * b.B, st) != 0) {
            hipStreamSynchronize(st);
            return VR_ERR_NO_DEVICE;
        }
    }
    const hipError_t e = hipMemcpyAsync(table, b.errTable, bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    return e != hipSuccess || es != hipSuccess ? VR_ERR_NO_DEVICE : VR_OK;
}

static vr_status assemble_common(bool toVolume, const uint8_t *src, int32_t nb, const int64_t bd[3], const int64_t *ijk,
                                 const int64_t grid[3], uint8_t *dst, void *stream)
{
    if (!src || !dst || !bd || !ijk || !grid || nb <= 0) return VR_ERR_INVALID;
    if (bd[0] % 16 != 0) return VR_ERR_UNSUPPORTED;
    if (nb > VR_MAX_BRICKS) return VR_ERR_UNSUPPORTED;   // k_assemble has the brick on gridDim.y
    for (int b = 0; b < nb; ++b)
        for (int k = 0; k < 3; ++k)
            if (ijk[3 * b + k] < 0 || ijk[3 * b + k] >= grid[k]) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    // the brick map lives on the device: uploaded once per distinct map and kept for the life of the process (a
    // streaming loop calls this every frame with the same map; allocating, copying and synchronising each time would
    // serialise the pipeline).  Cached maps are never freed, so a launch needs no lock; past 64 distinct maps a call
    // uploads its own copy and releases it after its launch has run.
    static std::mutex mu;
    static std::map<std::vector<int64_t>, int64_t *> cache;
    int64_t *d = nullptr;
    bool mine = false;
    {
        std::lock_guard<std::mutex> lk(mu);
        std::vector<int64_t> key(ijk, ijk + (size_t)nb * 3);
        int dev = 0;
        hipGetDevice(&dev);
        key.push_back(dev);
        auto it = cache.find(key);
        if (it == cache.end()) {
            HIPCHK(hipMalloc(&d, (size_t)nb * 3 * sizeof(int64_t)));
            if (hipMemcpy(d, ijk, (size_t)nb * 3 * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); return VR_ERR_NO_DEVICE; }
            if (cache.size() < 64) cache.emplace(std::move(key), d);
            else mine = true;
        } else d = it->second;
    }
    const int rc = assemble_launch(toVolume, src, dst, nb, bd, d, grid, (hipStream_t)stream);
    if (mine) { hipStreamSynchronize((hipStream_t)stream); hipFree(d); }
    return rc == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

vr_status vr_assemble_bricks(const uint8_t *bricks, int32_t nb, const int64_t bd[3], const int64_t *ijk,
                             const int64_t grid[3], uint8_t *volume, void *stream)
{
    return assemble_common(true, bricks, nb, bd, ijk, grid, volume, stream);
}
vr_status vr_disassemble_bricks(const uint8_t *volume, int32_t nb, const int64_t bd[3], const int64_t *ijk,
                                const int64_t grid[3], uint8_t *bricks, void *stream)
{
    return assemble_common(false, volume, nb, bd, ijk, grid, bricks, stream);
}

// The checks of the ray-casting entry points, each written once.  A frame: the camera, params and output, a positive
// size and max_samples >= 0.
static bool frame_ok(const vr_camera *cam, const vr_render_params *P, const float *rgba)
{
    return cam && P && rgba && P->width > 0 && P->height > 0 && P->max_samples >= 0;
}

// a dense volume: tex3d clamps to [0, X-1] (-1 for X = 0) and the launch narrows the extents to int
static bool dense_ok(const uint8_t *vol, const int64_t dims[3])
{
    if (!vol || !dims) return false;
    for (int k = 0; k < 3; ++k) if (dims[k] <= 0 || dims[k] >= (1ll << 31)) return false;
    return true;
}

// the virtual volume of a pool: power-of-two bricks, extents below 2^31 (tex3d's int indices); the table 16-byte
// aligned (pool_cell loads an entry as one uint4)
static bool pool_ok(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3])
{
    if (!pool || !table || !bd || !grid) return false;
    if (((uintptr_t)table & 15u) != 0) return false;
    for (int k = 0; k < 3; ++k) {
        if (bd[k] <= 0 || (bd[k] & (bd[k] - 1)) != 0 || grid[k] <= 0) return false;
        if (grid[k] >= (1ll << 31) / bd[k]) return false;
    }
    return true;
}

// a pool is the whole volume: no slab origin, and global_dims (if given) its extents
static bool pool_frame_ok(const vr_render_params *P, const int64_t bd[3], const int64_t grid[3])
{
    for (int k = 0; k < 3; ++k) {
        if (P->vol_origin[k] != 0) return false;
        if (P->global_dims[k] != 0 && P->global_dims[k] != grid[k] * bd[k]) return false;
    }
    return true;
}

// the transfer function's table (vrhip.h)
static bool table_ok(const vr_transfer_function *tf)
{
    if (!tf || !tf->lut_dev || ((uintptr_t)tf->lut_dev & 15u) != 0u) return false;
    if (!(tf->opacity_unit >= 0.0f) || !isfinite(tf->opacity_unit)) return false;
    for (int k = 0; k < 3; ++k) if (!isfinite(tf->background[k])) return false;
    return true;
}

static bool lighting_ok(const vr_shading *sh)
{
    if (!sh) return false;
    const float nonneg[5] = {sh->ambient, sh->diffuse, sh->specular, sh->shininess, sh->grad_min};
    for (int k = 0; k < 5; ++k) if (!(nonneg[k] >= 0.0f) || !isfinite(nonneg[k])) return false;
    for (int k = 0; k < 3; ++k) if (!isfinite(sh->light_dir[k])) return false;
    return true;
}

// The style is the entry point's, not a consequence of which pointers are null: greyscale (vr_raycast*) takes modes
// 0..2, a table (vr_raycast*_tf) VR_RENDER_COMPOSITE, lit (vr_raycast*_tf_shaded) VR_RENDER_SHADED and the lighting.
enum Style { GREY, TABLE, LIT };
static bool style_ok(Style s, const vr_render_params *P, const vr_transfer_function *tf, const vr_shading *sh)
{
    if (s == GREY) return P->mode >= 0 && P->mode <= 2;
    if (s == TABLE) return table_ok(tf) && P->mode == VR_RENDER_COMPOSITE;
    return table_ok(tf) && P->mode == VR_RENDER_SHADED && lighting_ok(sh);
}

// partial (TABLE and LIT only): rgba receives the colour partial of vr_raycast_tf_partial instead of the frame
static vr_status raycast_dense(Style s, const uint8_t *vol, const int64_t dims[3], const vr_camera *cam,
                               const vr_render_params *P, const vr_transfer_function *tf, const vr_shading *sh, float *rgba,
                               void *stream, bool partial = false)
{
    if (!frame_ok(cam, P, rgba) || !dense_ok(vol, dims) || !style_ok(s, P, tf, sh)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return raycast_launch(vol, dims, cam, P, tf, sh, partial, rgba, (hipStream_t)stream) == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

static vr_status raycast_pool(Style s, const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3],
                              const int64_t grid[3], const vr_camera *cam, const vr_render_params *P,
                              const vr_transfer_function *tf, const vr_shading *sh, float *rgba, void *stream,
                              bool partial = false)
{
    if (!frame_ok(cam, P, rgba) || !pool_ok(pool, table, bd, grid) || !pool_frame_ok(P, bd, grid) || !style_ok(s, P, tf, sh))
        return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return raycast_pool_launch(pool, table, bd, grid, cam, P, tf, sh, partial, rgba, (hipStream_t)stream) == 0 ? VR_OK
                                                                                                              : VR_ERR_NO_DEVICE;
}

vr_status vr_raycast(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                     float *rgba, void *stream)
{
    return raycast_dense(GREY, vol, dims, cam, P, nullptr, nullptr, rgba, stream);
}

vr_status vr_raycast_pool(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3],
                          const vr_camera *cam, const vr_render_params *P, float *rgba, void *stream)
{
    return raycast_pool(GREY, pool, table, bd, grid, cam, P, nullptr, nullptr, rgba, stream);
}

vr_status vr_raycast_tf(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                        const vr_transfer_function *tf, float *rgba, void *stream)
{
    return raycast_dense(TABLE, vol, dims, cam, P, tf, nullptr, rgba, stream);
}

vr_status vr_raycast_pool_tf(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3],
                             const vr_camera *cam, const vr_render_params *P, const vr_transfer_function *tf, float *rgba,
                             void *stream)
{
    return raycast_pool(TABLE, pool, table, bd, grid, cam, P, tf, nullptr, rgba, stream);
}

vr_status vr_raycast_tf_shaded(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                               const vr_transfer_function *tf, const vr_shading *sh, float *rgba, void *stream)
{
    return raycast_dense(LIT, vol, dims, cam, P, tf, sh, rgba, stream);
}

vr_status vr_raycast_pool_tf_shaded(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3],
                                    const vr_camera *cam, const vr_render_params *P, const vr_transfer_function *tf,
                                    const vr_shading *sh, float *rgba, void *stream)
{
    return raycast_pool(LIT, pool, table, bd, grid, cam, P, tf, sh, rgba, stream);
}

// the colour partial of the unlit (shading == NULL, VR_RENDER_COMPOSITE) or lit (VR_RENDER_SHADED) frame
vr_status vr_raycast_tf_partial(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                                const vr_transfer_function *tf, const vr_shading *sh, float *partial, void *stream)
{
    return raycast_dense(sh ? LIT : TABLE, vol, dims, cam, P, tf, sh, partial, stream, true);
}

vr_status vr_raycast_pool_tf_partial(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3],
                                     const int64_t grid[3], const vr_camera *cam, const vr_render_params *P,
                                     const vr_transfer_function *tf, const vr_shading *sh, float *partial, void *stream)
{
    return raycast_pool(sh ? LIT : TABLE, pool, table, bd, grid, cam, P, tf, sh, partial, stream, true);
}

// ---- two-dimensional transfer functions (vrhip.h) ---------------------------------------------------------------------
static bool table2d_ok(const float *lut, int32_t rows)
{
    return lut && ((uintptr_t)lut & 15u) == 0u && rows >= 2 && rows <= VR_TF2D_MAX_ROWS;
}

// the table, its scale and (where params attach a skip grid) its column summary; the mode is VR_RENDER_SHADED lit or not
static bool style2d_ok(const vr_render_params *P, const vr_transfer_function2d *tf, const vr_shading *sh)
{
    if (!tf || !table2d_ok(tf->lut_dev, tf->rows)) return false;
    if (((uintptr_t)tf->columns_dev & 15u) != 0u) return false;
    if (!tf->columns_dev && P->skip_grid_dev && P->skip_cell > 0) return false;
    if (!(tf->grad_scale > 0.0f) || !isfinite(tf->grad_scale)) return false;
    if (!(tf->opacity_unit >= 0.0f) || !isfinite(tf->opacity_unit)) return false;
    for (int k = 0; k < 3; ++k) if (!isfinite(tf->background[k])) return false;
    if (sh && !lighting_ok(sh)) return false;
    return P->mode == VR_RENDER_SHADED;
}

static vr_status raycast_dense2d(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                                 const vr_transfer_function2d *tf, const vr_shading *sh, float *rgba, void *stream, bool partial)
{
    if (!frame_ok(cam, P, rgba) || !dense_ok(vol, dims) || !style2d_ok(P, tf, sh)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return raycast_tf2d_launch(vol, dims, cam, P, tf, sh, partial, rgba, (hipStream_t)stream) == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

static vr_status raycast_pool2d(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3],
                                const vr_camera *cam, const vr_render_params *P, const vr_transfer_function2d *tf,
                                const vr_shading *sh, float *rgba, void *stream, bool partial)
{
    if (!frame_ok(cam, P, rgba) || !pool_ok(pool, table, bd, grid) || !pool_frame_ok(P, bd, grid) || !style2d_ok(P, tf, sh))
        return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return raycast_pool_tf2d_launch(pool, table, bd, grid, cam, P, tf, sh, partial, rgba, (hipStream_t)stream) == 0
               ? VR_OK : VR_ERR_NO_DEVICE;
}

vr_status vr_tf2d_columns_build(const float *lut, int32_t rows, uint16_t *columns, void *stream)
{
    if (!table2d_ok(lut, rows) || !columns || ((uintptr_t)columns & 15u) != 0u) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return tf2d_columns_launch(lut, rows, columns, (hipStream_t)stream) == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

vr_status vr_raycast_tf2d(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                          const vr_transfer_function2d *tf, const vr_shading *sh, float *rgba, void *stream)
{
    return raycast_dense2d(vol, dims, cam, P, tf, sh, rgba, stream, false);
}

vr_status vr_raycast_pool_tf2d(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3],
                               const vr_camera *cam, const vr_render_params *P, const vr_transfer_function2d *tf,
                               const vr_shading *sh, float *rgba, void *stream)
{
    return raycast_pool2d(pool, table, bd, grid, cam, P, tf, sh, rgba, stream, false);
}

vr_status vr_raycast_tf2d_partial(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                                  const vr_transfer_function2d *tf, const vr_shading *sh, float *partial, void *stream)
{
    return raycast_dense2d(vol, dims, cam, P, tf, sh, partial, stream, true);
}

vr_status vr_raycast_pool_tf2d_partial(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3],
                                       const int64_t grid[3], const vr_camera *cam, const vr_render_params *P,
                                       const vr_transfer_function2d *tf, const vr_shading *sh, float *partial, void *stream)
{
    return raycast_pool2d(pool, table, bd, grid, cam, P, tf, sh, partial, stream, true);
}

vr_status vr_skip_grid_build(const uint8_t *vol, const int64_t dims[3], int32_t cell, uint8_t *grid, void *stream)
{
    if (!dense_ok(vol, dims) || !grid || cell <= 0 || cell > 64) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return skip_grid_launch(vol, dims, cell, grid, (hipStream_t)stream) == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

vr_status vr_skip_grid_build_pool(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3],
                                  int32_t cell, uint8_t *out, void *stream)
{
    if (!pool_ok(pool, table, bd, grid) || !out || cell <= 0 || cell > 64) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return skip_grid_pool_launch(pool, table, bd, grid, cell, out, (hipStream_t)stream) == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

// ---- compositing of partial images: nine entry points, three kinds (PartialKind, raymarch.h)

// the combine calls read tf->background only: a null lut_dev is allowed
static bool background_ok(const vr_transfer_function *tf)
{
    if (!tf) return false;
    for (int k = 0; k < 3; ++k) if (!isfinite(tf->background[k])) return false;
    return true;
}

// an element-wise call: two images (front and back, or partial and frame) of n pixels
static bool images_ok(const float *a, const float *b, int64_t n) { return a && b && n > 0; }

// a slab call of an ordered kind: num_slabs partials of the num_pixels pixels from first_pixel on of cam's frame
static bool slab_tile_ok(const float *partials, int32_t num_slabs, int64_t num_pixels, int64_t first_pixel, int32_t axis,
                         const vr_camera *cam, const vr_render_params *P, const float *rgba)
{
    if (!partials || !cam || !P || !rgba || num_slabs <= 0 || num_pixels <= 0 || first_pixel < 0 || axis < 0 || axis > 2)
        return false;
    return P->width > 0 && P->height > 0 && first_pixel + num_pixels <= (int64_t)P->width * P->height;
}

static vr_status launched(int rc) { return rc == 0 ? VR_OK : VR_ERR_NO_DEVICE; }

vr_status vr_composite_over(float *front, const float *back, int64_t n, void *stream)
{
    if (!images_ok(front, back, n)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return launched(composite_over_launch({PartialKind::GREY}, front, back, n, (hipStream_t)stream));
}
vr_status vr_composite_finish(const float *partial, float *rgba, int64_t n, void *stream)
{
    if (!images_ok(partial, rgba, n)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return launched(composite_finish_launch({PartialKind::GREY}, partial, rgba, n, (hipStream_t)stream));
}
vr_status vr_composite_slabs(const float *partials, int32_t num_slabs, int64_t num_pixels, int64_t first_pixel, int32_t axis,
                             const vr_camera *cam, const vr_render_params *P, float *rgba, void *stream)
{
    if (!slab_tile_ok(partials, num_slabs, num_pixels, first_pixel, axis, cam, P, rgba)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return launched(composite_slabs_launch({PartialKind::GREY}, partials, num_slabs, num_pixels, first_pixel, axis, cam, P, rgba,
                                           (hipStream_t)stream));
}

vr_status vr_composite_over_tf(float *front, const float *back, int64_t n, void *stream)
{
    if (!images_ok(front, back, n)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return launched(composite_over_launch({PartialKind::COLOUR}, front, back, n, (hipStream_t)stream));
}
vr_status vr_composite_finish_tf(const float *partial, const vr_transfer_function *tf, float *rgba, int64_t n, void *stream)
{
    if (!images_ok(partial, rgba, n) || !background_ok(tf)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return launched(composite_finish_launch({PartialKind::COLOUR, tf}, partial, rgba, n, (hipStream_t)stream));
}
vr_status vr_composite_slabs_tf(const float *partials, int32_t num_slabs, int64_t num_pixels, int64_t first_pixel, int32_t axis,
                                const vr_camera *cam, const vr_render_params *P, const vr_transfer_function *tf, float *rgba,
                                void *stream)
{
    if (!slab_tile_ok(partials, num_slabs, num_pixels, first_pixel, axis, cam, P, rgba) || !background_ok(tf)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return launched(composite_slabs_launch({PartialKind::COLOUR, tf}, partials, num_slabs, num_pixels, first_pixel, axis, cam, P,
                                           rgba, (hipStream_t)stream));
}

// ---- intensity projections (vrhip.h): the entry points

static bool projection_frame_ok(const vr_render_params *P, const vr_projection *pj)
{
    return P->mode == VR_RENDER_PROJECTION && P->max_samples <= (1 << 24) && projection_ok(pj);
}

static vr_status project_dense(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                               const vr_projection *pj, float *rgba, void *stream, bool partial)
{
    if (!frame_ok(cam, P, rgba) || !dense_ok(vol, dims) || !projection_frame_ok(P, pj)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return raycast_proj_launch(vol, dims, cam, P, pj, partial, rgba, (hipStream_t)stream) == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

static vr_status project_pool(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3],
                              const vr_camera *cam, const vr_render_params *P, const vr_projection *pj, float *rgba,
                              void *stream, bool partial)
{
    if (!frame_ok(cam, P, rgba) || !pool_ok(pool, table, bd, grid) || !pool_frame_ok(P, bd, grid) || !projection_frame_ok(P, pj))
        return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return raycast_pool_proj_launch(pool, table, bd, grid, cam, P, pj, partial, rgba, (hipStream_t)stream) == 0 ? VR_OK
                                                                                                               : VR_ERR_NO_DEVICE;
}

vr_status vr_raycast_projection(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                                const vr_projection *pj, float *rgba, void *stream)
{
    return project_dense(vol, dims, cam, P, pj, rgba, stream, false);
}

vr_status vr_raycast_pool_projection(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3], const int64_t grid[3],
                                     const vr_camera *cam, const vr_render_params *P, const vr_projection *pj, float *rgba,
                                     void *stream)
{
    return project_pool(pool, table, bd, grid, cam, P, pj, rgba, stream, false);
}

vr_status vr_raycast_projection_partial(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam,
                                        const vr_render_params *P, const vr_projection *pj, float *partial, void *stream)
{
    return project_dense(vol, dims, cam, P, pj, partial, stream, true);
}

vr_status vr_raycast_pool_projection_partial(const uint8_t *pool, const vr_pool_entry *table, const int64_t bd[3],
                                             const int64_t grid[3], const vr_camera *cam, const vr_render_params *P,
                                             const vr_projection *pj, float *partial, void *stream)
{
    return project_pool(pool, table, bd, grid, cam, P, pj, partial, stream, true);
}

vr_status vr_composite_combine_proj(float *front, const float *back, int64_t n, int32_t op, void *stream)
{
    if (!images_ok(front, back, n) || op < VR_PROJECT_MAX || op > VR_PROJECT_MEAN) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    vr_projection pj = {};      // a fold reads the op alone
    pj.op = op;
    return launched(composite_over_launch({PartialKind::PROJECTION, nullptr, &pj}, front, back, n, (hipStream_t)stream));
}
vr_status vr_composite_finish_proj(const float *partial, const vr_projection *pj, float *rgba, int64_t n, void *stream)
{
    if (!images_ok(partial, rgba, n) || !projection_ok(pj)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return launched(composite_finish_launch({PartialKind::PROJECTION, nullptr, pj}, partial, rgba, n, (hipStream_t)stream));
}
vr_status vr_composite_slabs_proj(const float *partials, int32_t num_slabs, int64_t num_pixels, const vr_projection *pj,
                                  float *rgba, void *stream)
{
    if (!images_ok(partials, rgba, num_pixels) || num_slabs <= 0 || !projection_ok(pj)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return launched(composite_slabs_launch({PartialKind::PROJECTION, nullptr, pj}, partials, num_slabs, num_pixels, 0, 0, nullptr,
                                           nullptr, rgba, (hipStream_t)stream));
}

// ---- slice views (vrhip.h): the entry points

// a vr_slice_plane (vrhip.h): the sizes, the filter and finite geometry
static bool plane_ok(const vr_slice_plane *pl)
{
    if (!pl || pl->width <= 0 || pl->height <= 0 || pl->layers < 1 || pl->layers > (1 << 24)) return false;
    if (pl->filter != VR_SLICE_NEAREST && pl->filter != VR_SLICE_LINEAR) return false;
    for (int k = 0; k < 3; ++k)
        if (!isfinite(pl->origin[k]) || !isfinite(pl->du[k]) || !isfinite(pl->dv[k]) || !isfinite(pl->dw[k]) ||
            !isfinite(pl->box_min[k]) || !isfinite(pl->box_max[k]))
            return false;
    return true;
}

static vr_status slice_dense(const uint8_t *vol, const int64_t dims[3], const vr_slice_plane *pl, const vr_projection *pj,
                             float *out, void *stream, bool partial)
{
    if (!out || !dense_ok(vol, dims) || !plane_ok(pl) || !projection_ok(pj)) return VR_ERR_INVALID;
    if (!device_ok()) return VR_ERR_NO_DEVICE;
    return reslice_launch(vol, dims, pl, pj, partial, out, (hipStream_t)stream) == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

vr_status vr_reslice(const uint8_t *vol, const int64_t dims[3], const vr_slice_plane *pl, const vr_projection *pj, float *rgba,
                     void *stream)
{
    return slice_dense(vol, dims, pl, pj, rgba, stream, false);
}

vr_status vr_reslice_partial(const uint8_t *vol, const int64_t dims[3], const vr_slice_plane *pl, const vr_projection *pj,
                             float *partial, void *stream)
{
    return slice_dense(vol, dims, pl, pj, partial, stream, true);
}

vr_status vr_brickset_set_concurrency(vr_brickset *h, int32_t level_loop_streams)
{
    if (!h || level_loop_streams < 1 || level_loop_streams > 4) return VR_ERR_INVALID;
    h->s.levelLoopStreams = level_loop_streams;
    return VR_OK;
}

vr_status vr_brickset_last_timings(vr_brickset *h, float ms[5])
{
    if (!h || !ms) return VR_ERR_INVALID;
    BrickSet &b = h->s;
    if (b.timingsPending) {
        HIPCHK(hipEventSynchronize(b.ev[4]));
        for (int i = 0; i < 4; ++i) hipEventElapsedTime(&b.phasesMs[i], b.ev[i], b.ev[i + 1]);
        b.timingsPending = false;
    }
    if (b.decodeTimingPending) {
        HIPCHK(hipEventSynchronize(b.ev[6]));
        hipEventElapsedTime(&b.phasesMs[4], b.ev[5], b.ev[6]);
        b.decodeTimingPending = false;
    }
    for (int i = 0; i < 5; ++i) ms[i] = b.phasesMs[i];
    return VR_OK;
}

} // extern "C"
