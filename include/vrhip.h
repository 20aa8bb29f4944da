/*
 * vrhip.h -- C ABI of the MI355X-native kd-tree volume codec + ray-march compositor.
 *
 * This is the drop-in boundary for ONE hot path of AugmentariumLab/VolumeRenderer:
 *   ingest   VolumeReader<T>::LoadBricksToTexture        volume_renderer/VolumeReader.h:151-223
 *   encode   VolumeKdtree::build                          volume_renderer/VolumeKdTree_recover.cpp:17-140
 *   decode   VolumeKdtree::levelCut                       volume_renderer/VolumeKdTree_recover.cpp:726-835
 *   file     VolumeKdtree::save / open                    volume_renderer/VolumeKdTree_recover.cpp:521-594
 *   4-bit    MidRangeTree::build / convertToByteArray     volume_renderer/MidRangeTree.cpp:17-176,1095-1128
 *   render   raycaster.frag / isosurface.frag + UnitBrick::Draw
 *                                                         volume_renderer/raycaster.frag:18-86,
 *                                                         volume_renderer/isosurface.frag:77-159,
 *                                                         volume_renderer/UnitBrick.h:98-100
 * The reference has no FFI layer; its boundary is the public surface of those C++
 * classes, called from main.cpp:142-290,358-404.  The headers in include/vrhip/ re-create
 * that surface (same class and method names) as a header-only facade over the
 * functions below.  Everything behind this header is hand-written HIP for gfx950;
 * there is NO CPU fallback: every compute entry point returns VR_ERR_NO_DEVICE
 * when no HIP device is usable.
 *
 * Conventions
 *  - plain C, no exceptions across the boundary, every function returns vr_status;
 *  - volumes are uint8, x fastest: cell(x,y,z) = x + X*y + X*Y*z (R.cpp:4-6);
 *  - "dev" pointers are HIP device pointers, "host" pointers ordinary memory;
 *    the caller owns every buffer it passes;
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls
 *    that return data to the host synchronise that stream before returning;
 *    device-to-device calls are asynchronous on it.
 *  - a vr_brickset is a batch of B independent bricks of identical dimensions, one
 *    kd-tree per brick (a single VolumeKdtree is a brickset with B = 1).  All B
 *    trees are built / decoded by the same batched kernel launches.
 *  - alignment of caller buffers.  Host pointers and the render half's device buffers may start at any byte unless
 *    their entry says otherwise.  The codec's fastest kernels touch the caller's device buffer with 16-byte (the pool
 *    packer: 4-byte) vectors, and the library does not rely on the hardware's tolerance of misaligned vector accesses:
 *    a call that would launch such a kernel on a buffer that is not 16-byte aligned returns VR_ERR_INVALID with nothing
 *    launched, nothing written and the set unchanged (as for vr_transfer_function::lut_dev); the same call with an
 *    aligned buffer then works as ever.  Every other call takes its buffers at any byte offset and writes exactly the
 *    bytes its entry names.  Each codec entry point below states its rule in a line that begins "Alignment:".  Two
 *    terms, for power-of-two extents up to 1024 per axis (a set created under VRHIP_FORCE_IDX64 has neither):
 *      x-run geometry: orig_tree_depth >= 12 and at least four of the twelve deepest tree levels split x -- e.g.
 *        16x16x16, 16x8x32, 128x8x4, every cube from 16 up, the reference's brick sizes; not 8x64x64;
 *      tiled geometry: X >= 128 and the six deepest tree levels split each axis twice in one repeated order, which is
 *        (log2 X, log2 Y, log2 Z) = (m, m, m), (m+1, m, m) or (m+1, m+1, m) -- 128x64x64, 128x128x64, 128^3, 256x128x128,
 *        256x256x128, 256^3 ...; not 128x8x4, 128x32x16 or 64^3.
 *    Bricks of either geometry hold a multiple of 16 voxels, so every brick of an aligned buffer is aligned.
 */
#ifndef VRHIP_H
#define VRHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t vr_status;
enum {
    VR_OK = 0,
    VR_ERR_INVALID = -1,     /* bad argument (null pointer, non-positive dims, negative tolerance ...) */
    VR_ERR_NO_DEVICE = -2,   /* no usable HIP device / HIP call failed; there is no CPU fallback */
    VR_ERR_OOM = -3,
    VR_ERR_IO = -4,          /* save/open: file missing or short (reference: exit(-1), R.cpp:560-565) */
    VR_ERR_STATE = -5,       /* e.g. decode before build, save of an empty tree (R.cpp:526-530) */
    VR_ERR_FORMAT = -6,      /* malformed tree stream */
    VR_ERR_UNSUPPORTED = -7
};

/* Which reference class the brickset mirrors. */
enum {
    VR_VARIANT_RECOVER = 0,  /* VolumeKdTree_recover.cpp (live copy)                         */
    VR_VARIANT_GUARDED = 1,  /* VolumeKdtree.cpp:333 guard -- byte-identical output, less work */
    VR_VARIANT_MIDRANGE = 2  /* MidRangeTree.cpp: second 2-bit stream + 4-bit packing         */
};

typedef struct vr_brickset vr_brickset;

/* Mirrors the public data members of class VolumeKdtree (VolumeKdtree_recover.h:57-79). */
typedef struct vr_tree_info {
    int64_t X, Y, Z;             /* brick dimensions                               */
    int32_t orig_tree_depth;     /* origTreeDepth  (R.cpp:29)                      */
    int32_t max_tree_depth;      /* maxTreeDepth = orig + 7 (R.cpp:30)             */
    int64_t num_active_nodes;    /* numActiveNodes (R.cpp:714)                     */
    int64_t tree_bytes;          /* tree.bytes() = ceil(numActiveNodes / 4)        */
    int32_t tolerance, max_epochs, variant;
    int32_t num_reverts;         /* gradient-descent reverts taken (defect C-2 indicator); MidRangeTree: both streams' */
    int32_t max_error_before;    /* encoder's own leaf max error before branch growth (R.cpp:71-76) */
    int32_t max_error_after;     /* ... after branch growth (R.cpp:115-120)        */
    double  mean_l1_after;       /* (R.cpp:122-129)                                */
    int32_t zero_run_rewrites;   /* grown branches that ended on an evaluated "keep": the reference rewrites such a run
                                  * of zeros to 3s (R.cpp:662-669,686-688).  Provably impossible for tolerance >= 0, so
                                  * the GPU emitters count instead of rewriting; anything but 0 here means the stream
                                  * differs from the reference's */
    int32_t est_exact_segments;  /* diagnostic: 1024-node segments the distance estimator (R.cpp:415-455) had to walk node by
                                  * node instead of taking from their summaries; 0 for opened / set trees */
} vr_tree_info;

/* ---- library / device ------------------------------------------------------- */
vr_status vr_device_count(int32_t *count);                 /* VR_OK + 0 devices is possible (CPU-only box) */
vr_status vr_set_device(int32_t device);
const char *vr_status_string(vr_status s);
const char *vr_version(void);

/* ---- device buffers for host code that does not include HIP headers ----------------
 * (the reference's host code hands over std::vector<byte>; the facade in include/vrhip/
 * stages it through these).  Copies synchronise `stream` before returning. */
vr_status vr_malloc(void **dev, int64_t bytes);
vr_status vr_free(void *dev);
vr_status vr_upload(void *dst_dev, const void *src_host, int64_t bytes, void *stream);
vr_status vr_download(void *dst_host, const void *src_dev, int64_t bytes, void *stream);

/* ---- brickset life cycle ------------------------------------------------------
 * VolumeKdtree(std::vector<byte>&, x, y, z) + setErrorTolerance + setMaxEpochs
 * (VolumeKdtree_recover.h:103-112, R.cpp:9-15).  Any extents are accepted, as in the reference
 * (R.cpp:26-36: origTreeDepth = the sum of the floors of the three log2; R.cpp:151-162: the split rule that
 * follows from it -- unequal halves, an axis order that differs from node to node, leaves that read the min
 * corner of a box of several cells, R.cpp:194-195, and levelCut's boxes that leave some voxels unwritten,
 * R.cpp:759-766 with 806-833; all reproduced bit for bit).  Power-of-two extents up to 1024 per axis (the
 * reference's brick sizes 256x256x128 / 256^3) take the tiled fast kernels, everything else table-driven ones.
 * Limits of one tree: origTreeDepth <= 31, fewer than 2^32 voxels and at most 2^20 cells per axis; deeper than 28
 * levels (a stream can then pass 2^32 tokens: 64-bit token offsets, table-driven kernels) only with num_bricks == 1
 * -> VR_ERR_UNSUPPORTED beyond.  The reference program's own 2048x2048x768 tree (main.cpp:242-251) is 31 levels.
 * tolerance: any non-negative value.  A leaf error never exceeds 255, so every tolerance >= 256 means the same thing:
 * the kernels are given min(tolerance, 256); vr_brickset_info keeps reporting the caller's value.
 * max_epochs: 0 .. VR_MAX_EPOCHS.  A build issues max_epochs x origTreeDepth x (3 to 4) launches whatever the data
 * does (no level used more than 13 epochs on the volumes measured), so a larger value is refused
 * with VR_ERR_UNSUPPORTED by vr_brickset_create and vr_brickset_set_max_epochs (the set then keeps its setting),
 * before anything is launched.
 * num_bricks: 1 .. VR_MAX_BRICKS.  The batched launches carry the brick index on the grid's second axis, which the
 * device limits (an MI355X reports 65536); a larger set is refused with VR_ERR_UNSUPPORTED here, before the device is
 * touched, and nothing is ever launched past that limit. */
#define VR_MAX_EPOCHS 1024
#define VR_MAX_BRICKS 65535
vr_status vr_brickset_create(vr_brickset **out, int32_t num_bricks, const int64_t dims[3],
                             int32_t tolerance, int32_t max_epochs, int32_t variant);
vr_status vr_brickset_destroy(vr_brickset *bs);
vr_status vr_brickset_set_error_tolerance(vr_brickset *bs, int32_t tolerance);   /* R.cpp:9-11  */
vr_status vr_brickset_set_max_epochs(vr_brickset *bs, int32_t max_epochs);       /* R.cpp:13-15 */

/* ---- encode: VolumeKdtree::build (R.cpp:17-140) --------------------------------
 * voxels_dev: num_bricks * X*Y*Z bytes, brick b at offset b*X*Y*Z, each x-fastest.
 * Unlike the reference (R.cpp:51-52) the input buffer is left untouched.
 * Asynchronous on `stream`; vr_brickset_info()/get_* synchronise.
 * Alignment: x-run geometry: voxels_dev 16-byte aligned, else VR_ERR_INVALID (the set keeps its previous trees); any
 * other set: any byte offset. */
vr_status vr_brickset_build(vr_brickset *bs, const uint8_t *voxels_dev, void *stream);

/* Public members after build(): per-brick info, tree bytes (TwoBitArray::bits of
 * the preorder stream), distanceMap (maxTreeDepth+1 bytes). */
vr_status vr_brickset_info(vr_brickset *bs, int32_t brick, vr_tree_info *info);
vr_status vr_brickset_get_tree(vr_brickset *bs, int32_t brick, uint8_t *dst_host, int64_t capacity);
vr_status vr_brickset_get_distance_map(vr_brickset *bs, int32_t brick, uint8_t *dst_host, int32_t capacity);
/* MidRangeTree only: tree_range.bits, distanceMap_range, convertToByteArray (M.cpp:1095-1128);
 * packed length is returned through *length (pass dst_host = NULL to query it). */
vr_status vr_brickset_get_tree_range(vr_brickset *bs, int32_t brick, uint8_t *dst_host, int64_t capacity);
vr_status vr_brickset_get_distance_map_range(vr_brickset *bs, int32_t brick, uint8_t *dst_host, int32_t capacity);
vr_status vr_brickset_get_packed4(vr_brickset *bs, int32_t brick, uint8_t *dst_host, int64_t capacity, int64_t *length);

/* ---- decode: VolumeKdtree::levelCut (R.cpp:726-835) ----------------------------
 * out_dev: num_bricks * X*Y*Z bytes.  cut_depth == max_tree_depth (or < 0) is the reference's
 * levelCut, bit-exact.  0 <= cut_depth < max_tree_depth is a PROGRESSIVE cut with defined
 * semantics (new: the reference's walk de-synchronises there): the stream is
 * parsed completely, refinement stops below the cut, every voxel gets the decoded scalar of its
 * ancestor at depth min(cut_depth, depth of its terminal node).  Asynchronous on `stream`.
 * Alignment: tiled geometry: out_dev 16-byte aligned at every cut, else VR_ERR_INVALID; any other set: any byte
 * offset.  Exactly num_bricks * X*Y*Z bytes are written. */
vr_status vr_brickset_decode(vr_brickset *bs, int32_t cut_depth, uint8_t *out_dev, void *stream);

/* Per-brick progressive decode (view-dependent level of detail).  cuts_host[b] for every brick b of the set:
 *   -1                      brick b is skipped: its X*Y*Z bytes of out_dev are left untouched
 *   0 .. max_tree_depth     brick b is decoded exactly as vr_brickset_decode(bs, cuts_host[b], ...) decodes it
 * Any other value -> VR_ERR_INVALID (nothing launched).  Asynchronous on `stream`; cuts_host may be reused as soon
 * as the call returns.  The bricks are grouped by the kernel a uniform decode at their cut would use, one launch
 * per non-empty group; skipped bricks cost nothing.
 * Concurrency: each call has its own device lists, cut values and tables, taken from a ring of four per set.  Up to
 * four calls may be in flight, back to back on one stream or on several streams, without a host synchronisation; a
 * fifth waits on the host until the oldest has finished.  Calls on one set from several host threads at once are
 * not supported (no call on a set is).  A set opened from a file, cut above the index level, fills the cut values on
 * the host (as vr_brickset_decode does).  vr_brickset_last_timings reports the call's whole time as `decode`.
 * Alignment: tiled geometry with any cut >= 0: out_dev 16-byte aligned, else VR_ERR_INVALID; any other set, or every
 * brick skipped: any byte offset.  Only the X*Y*Z bytes of bricks with a cut >= 0 are written. */
vr_status vr_brickset_decode_lod(vr_brickset *bs, const int32_t *cuts_host, uint8_t *out_dev, void *stream);

/* Level-of-detail pool: each brick of a frame stored at the resolution its cut actually has.  For power-of-two brick
 * extents a progressive cut c is piecewise constant on the boxes of the depth-min(c, orig_tree_depth) nodes, so a
 * brick cut at c is kept as one byte per box with nothing lost.  One 16-byte entry per grid cell (x fastest): */
typedef struct vr_pool_entry {
    int64_t offset;      /* byte offset of the cell's brick in the pool; -1 = absent (culled, or no brick at the cell) */
    uint8_t shift[3];    /* log2 of the box one stored voxel stands for, per axis (0 = full resolution) */
    uint8_t pad[5];      /* 0 */
} vr_pool_entry;
/* The table contract of every pool reader (vr_raycast_pool and its _tf, _tf_shaded, _tf_partial, _tf2d, _tf2d_partial,
 * _projection and _projection_partial variants, vr_skip_grid_build_pool, vr_histogram_pool).  The pool and the table are
 * the caller's buffers and need not come from vr_brickset_decode_lod_pool:
 *  - table_dev 16-byte aligned, else VR_ERR_INVALID, nothing launched (the kernels load an entry as one 16-byte word;
 *    the struct's own alignment is only 8);
 *  - pool_dev at any byte, slots at any byte offset, in any order, back to back or apart; several cells may name one slot;
 *  - an entry with offset >= 0 has shift_k <= log2(brick_dims_k) on every axis and its slot, prod_k(brick_dims_k >>
 *    shift_k) bytes from pool_dev + offset, lies inside the pool; offset is a full 64-bit byte offset;
 *  - every negative offset reads as absent (the layout writes -1); an absent entry's shift and every pad are not read.
 * The entries live on the device and no entry point reads them on the host: the third point is the caller's to keep,
 * and a table that breaks it makes the kernels read outside the pool. */

/* Host-only: the pool layout of vr_brickset_decode_lod_pool.  Bricks as in vr_assemble_bricks (brick b of brick_dims
 * voxels at cell brick_ijk[3b..3b+2] of `grid`), cuts as in vr_brickset_decode_lod.  The rule:
 *  - split axes: depth d = 0, 1, ... splits axis sd = d % 3, or, while the box still has more than one voxel and
 *    extent 1 on sd, the next axis (d + 1) % 3, (d + 2) % 3 ...; the split halves that extent (the reference's
 *    buildRecursive).  n_k = the splits on axis k among depths 0 .. min(cut, orig_tree_depth) - 1.
 *  - shift_k = log2(brick_dims_k) - n_k; a cut >= orig_tree_depth gives shift 0 on every axis.
 *  - bricks are placed in index order b = 0 .. num_bricks-1: brick b with cuts[b] >= 0 gets offset = the running
 *    total rounded up to a multiple of 256, and adds prod_k(brick_dims_k >> shift_k) bytes to it.  The stored voxel
 *    (x, y, z) of a brick, x fastest, is brick voxel (x << shift_x, y << shift_y, z << shift_z): voxel (x, y, z) of the
 *    brick reads stored voxel (x >> shift_x, y >> shift_y, z >> shift_z).
 *  - cells with no brick, or whose brick has cut -1, get offset -1 and shift 0.  *pool_bytes = the final total (not
 *    rounded; 0 if every brick is culled).
 * VR_ERR_INVALID: a null pointer (table_out aside), num_bricks <= 0, a brick_dims extent that is not a power of two,
 * a grid extent <= 0, a brick outside the grid, two bricks on one cell, a cut outside -1 .. max_tree_depth, orig_tree_depth not the depth of
 * brick_dims (log2 X + log2 Y + log2 Z), or max_tree_depth < orig_tree_depth.  table_out may be NULL. */
vr_status vr_lod_pool_layout(const int64_t brick_dims[3], int32_t num_bricks, const int64_t *brick_ijk,
                             const int64_t grid[3], const int32_t *cuts, int32_t orig_tree_depth,
                             int32_t max_tree_depth, vr_pool_entry *table_out, int64_t *pool_bytes);

/* Per-brick progressive decode into a pool laid out by vr_lod_pool_layout (the set's dims, the same brick_ijk, grid
 * and cuts): brick b's stored voxel (x, y, z) = voxel (x << shift_x, y << shift_y, z << shift_z) of brick b in
 * vr_brickset_decode_lod's output for the same cuts, i.e. the box's min-corner voxel, which every voxel of the box
 * equals.  pool_bytes must be at least the layout's.  Pool bytes outside the slots of decoded bricks are not written.
 * table_dev (may be NULL): receives the layout's grid[0]*grid[1]*grid[2] entries, uploaded on `stream`.
 * Full-resolution bricks are decoded straight into their slots; coarse ones at most VR_POOL_STAGE_BRICKS at a time into
 * a staging buffer of the set, then packed.  The staging buffer's use is ordered across streams by an event; the
 * lists come from vr_brickset_decode_lod's ring (same concurrency contract, no host synchronisation).
 * VR_ERR_UNSUPPORTED (nothing launched) unless every brick extent is a power of two; VR_ERR_INVALID as for the layout
 * and for a pool smaller than the layout's.  vr_brickset_last_timings reports the call's whole time as `decode`.
 * Alignment: pool_dev 16-byte aligned, else VR_ERR_INVALID (the table is not uploaded either), when the set has tiled
 * geometry and a brick with cut >= 0 is stored at full resolution (shift 0 on every axis), or when a brick of any set
 * is stored coarser with rows of four stored voxels or more ((X >> shift_x) >= 4); otherwise any byte offset.  table_dev
 * is written by a copy: any byte offset. */
#define VR_POOL_STAGE_BRICKS 32
vr_status vr_brickset_decode_lod_pool(vr_brickset *bs, const int32_t *cuts_host, const int64_t *brick_ijk_host,
                                      const int64_t grid[3], uint8_t *pool_dev, int64_t pool_bytes,
                                      vr_pool_entry *table_dev, void *stream);

/* MidRangeTree only (new: the reference builds the half-range stream, MidRangeTree.cpp:399-544, 871-982, but
 * never decodes it -- its levelCut, :984-1093, reads the mid stream alone): the same progressive
 * decode applied to the range stream, i.e. per voxel the half range of its terminal node's box as the
 * encoder reconstructed it (distanceMap_range, codes of tree_range).  With vr_brickset_decode this gives
 * [mid - range, mid + range] bounds at any cut depth (coarse-to-fine refinement, empty-space tests).
 * VR_ERR_STATE for other variants, VR_ERR_UNSUPPORTED for a set opened from a file.
 * Alignment: as vr_brickset_decode. */
vr_status vr_brickset_decode_range(vr_brickset *bs, int32_t cut_depth, uint8_t *out_dev, void *stream);

/* Install a foreign preorder stream (e.g. read from a reference-written file) as
 * brick `brick`: builds the decode side-car index from the bytes alone.
 * Any stream of the grammar of SURVEY.md Appendix A.4 is accepted, with any distance
 * map: not only what an encoder emits (prunes at any depth, grown branches of any
 * length 0 .. 7, distances of any byte value).  vr_brickset_decode, _decode_lod and
 * _decode_lod_pool then give the values that grammar defines, at every cut
 * (_decode_lod_pool at power-of-two extents only: VR_ERR_UNSUPPORTED otherwise, with
 * nothing written, whatever installed the streams).  At extents that are not powers
 * of two, or longer than 1024, the boxes are those of the reference's levelCut: a
 * leaf box of several cells is halved once per node of its grown branch, the
 * terminating 3 included, only what is left is written and the other cells are 0,
 * at every cut (a cut stops the scalar updates, not the halvings).
 * A stream that ends early, has tokens left over or ends inside a grown branch is
 * VR_ERR_FORMAT and leaves the set as it was.  Every status other than VR_OK and a
 * device error (VR_ERR_NO_DEVICE) leaves the set unchanged, VR_ERR_OOM included.
 * Extents that the tiled decoders serve: k_decode_region and k_decode_quad hold the
 * grown-branch distances (map entries origTreeDepth + 1 .. + 7) as the constants
 * 64 >> i, so a brick whose map says otherwise is decoded by the walking kernel,
 * which reads them from the map, and one such brick sends its whole set there (the
 * results are the same).  Installing the brick again decides anew.  At all other
 * extents one kernel decodes every stream and reads the distances from the map.
 * A set may hold bricks that were never installed: vr_brickset_decode_lod and
 * _decode_lod_pool skip them with cut -1. */
vr_status vr_brickset_set_tree(vr_brickset *bs, int32_t brick, const uint8_t *tree_host, int64_t tree_bytes,
                               int64_t num_active_nodes, const uint8_t *distance_map_host, int32_t map_len);

/* ---- file format: VolumeKdtree::save / open (R.cpp:521-594) --------------------
 * Byte-identical to the reference's file: rootMin,rootMax (3x int64 each),
 * maxTreeDepth, origTreeDepth (int32), X,Y,Z,numActiveNodes (int64), distanceMap,
 * tree bytes.  vr_brickset_open creates a 1-brick set. */
vr_status vr_brickset_save(vr_brickset *bs, int32_t brick, const char *path);
vr_status vr_brickset_open(vr_brickset **out, const char *path);
/* MidRangeTree::save / open (MidRangeTree.cpp:753-833).  A VR_VARIANT_MIDRANGE set saves the
 * reference's MidRangeTree layout byte for byte: the same 88-byte header, distanceMap,
 * distanceMap_range, tree bytes, tree_range bytes.  vr_brickset_open_variant(…, VR_VARIANT_MIDRANGE)
 * reads such a file back exactly (the reference's reader mis-sizes the streams by 4 bytes and returns
 * a shifted range stream: nothing to match); other variants forward to vr_brickset_open. */
vr_status vr_brickset_open_variant(vr_brickset **out, const char *path, int32_t variant);

/* ---- compressed brick-set archives: stored streams installed on the GPU, and a file of one set -------------
 * vr_brickset_set_tree parses one stream on the host and installs it with blocking copies; the calls below install
 * many streams at once and rebuild the decode index on the GPU, in parallel, from a small seek table per stream.
 *
 * The block table of a stream, for a brick of depth D = origTreeDepth: Dc = max(D - 12, 0); a block is a depth-Dc
 * node (a 4096-leaf box where D >= 12, the whole brick otherwise); nBlk = 2^Dc.
 *   block_off[nBlk]      uint32: the token index of the block root's own token, 0xFFFFFFFF where an ancestor of
 *                        the root was pruned (the block is dead);
 *   top_val[2 nBlk]      uint8, a 1-based heap over depths 0 .. Dc: entry (1 << j) + path is the decoded scalar of
 *                        the depth-j node `path` (the root's is distance_map[0]; every token is applied with
 *                        distance_map[j] as the decoder does), or of its pruned ancestor where it does not exist.
 *                        Entry 0 is unused.
 * vr_stream_block_table makes the table of a stream on the host, with one pass over its tokens; it needs no device.
 * VR_ERR_FORMAT for a stream the grammar does not produce.
 *
 * vr_brickset_set_trees installs descs[i] as brick bricks[i] (no brick twice), for count bricks at once, into a
 * fresh set or one that holds installed streams only (a built set: VR_ERR_STATE); VR_VARIANT_MIDRANGE sets and sets
 * with 64-bit token offsets are VR_ERR_UNSUPPORTED.  Per stream, as for vr_brickset_set_tree: num_active below 2^32
 * (else VR_ERR_UNSUPPORTED), map_len >= maxTreeDepth + 1 (else VR_ERR_INVALID), tree_bytes >= (num_active + 3) / 4
 * bytes that fit the set's stream slots (else VR_ERR_FORMAT).  A desc with both table pointers null gets its table
 * from vr_stream_block_table here (slow: a host pass over the stream); one with one of them null is VR_ERR_INVALID.
 * A table is checked on the host before anything is enqueued (every live offset below num_active, live offsets
 * strictly increasing, block 0 at token Dc when live): VR_ERR_FORMAT, the set unchanged.  Then everything is enqueued
 * on `stream`: the copies, the reset of the named bricks' index entries, k_index_from_stream, which parses every token
 * of every named stream exactly once, and one synchronisation of `stream` at the end.  VR_OK, or VR_ERR_FORMAT if a
 * named stream is not of the grammar or disagrees with its table's offsets: then EVERY brick named in the call is left
 * "never installed" (bricks not named keep their state).  Wrong scalars in top_val are not detected: they give other
 * voxel values, nothing worse.  No input makes the kernel read or write outside its buffers or run forever.
 * The host pointers are read before the call returns.  No host copy of the streams is kept: decodes at cuts above the
 * index depth take their scalars from a heap the kernel wrote, without touching the host.  vr_brickset_info,
 * _get_tree, _get_distance_map and _save return the installed bytes and values; the rule about grown-branch distances
 * other than 64 >> i is vr_brickset_set_tree's. */
typedef struct vr_tree_desc {            /* host pointers */
    const uint8_t *tree; int64_t tree_bytes; int64_t num_active;
    const uint8_t *distance_map; int32_t map_len;
    const uint32_t *block_off; const uint8_t *top_val;
} vr_tree_desc;
vr_status vr_stream_block_table(const int64_t dims[3], const uint8_t *tree_host, int64_t tree_bytes, int64_t num_active,
                                const uint8_t *distance_map_host, int32_t map_len, uint32_t *block_off_out,
                                uint8_t *top_val_out);
vr_status vr_brickset_set_trees(vr_brickset *bs, int32_t count, const int32_t *bricks, const vr_tree_desc *descs,
                                void *stream);

/* The archive: one file holds one brick set (one timestep).  Little-endian; every section starts 16-byte aligned and
 * is zero-padded to a multiple of 16 bytes, so a file read into one pinned buffer is installed from it as it lies.
 *   header, 64 bytes     char magic[8] = "VRBSET\r\n"; uint32 version = 1; uint32 variant; int64 dims[3] (of a brick);
 *                        int32 num_bricks, origTreeDepth, maxTreeDepth; uint32 0; int64 file_bytes
 *   directory            num_bricks entries of 32 bytes: int64 offset of the brick's record from the start of the
 *                        file (0: the brick is absent), int64 tree_bytes = (num_active + 3) / 4, int64 num_active,
 *                        uint64 FNV-1a-64 of the record's bytes (padding included)
 *   record of a brick    distance_map[maxTreeDepth + 1], top_val[2 nBlk], block_off[nBlk], tree[tree_bytes]
 * vr_brickset_save_set writes a built set or a set of installed streams (VR_ERR_STATE for neither; VR_VARIANT_MIDRANGE:
 * VR_ERR_UNSUPPORTED); bricks never installed are absent.  The tables are made on the host, on at most 16 threads.
 * vr_brickset_open_set creates a set from a file (tolerance and max_epochs: vr_brickset_open's defaults) and installs
 * it; vr_brickset_load_set / _load_set_memory install a file / a file's bytes in host memory (16-byte aligned, else
 * VR_ERR_INVALID; pinned memory makes the copies asynchronous) into an existing set with vr_brickset_set_trees, every
 * brick of the file in one call; bricks absent from the file keep their state.  VR_ERR_FORMAT with the set unchanged,
 * before anything is enqueued: a wrong magic or version, a file_bytes that is not the size, geometry (variant, dims,
 * num_bricks, depths) that does not match the set, an offset or length outside the file, a checksum mismatch, a
 * table that fails vr_brickset_set_trees' host check.  VR_ERR_IO for a file that cannot be read or written. */
vr_status vr_brickset_save_set(vr_brickset *bs, const char *path);
vr_status vr_brickset_open_set(vr_brickset **out, const char *path, void *stream);
vr_status vr_brickset_load_set(vr_brickset *bs, const char *path, void *stream);
vr_status vr_brickset_load_set_memory(vr_brickset *bs, const void *blob_host, int64_t bytes, void *stream);

/* ---- error helpers: measureMaxError / measureMeanError / queryError (R.cpp:386-411)
 * The reference dereferences the input it has already cleared (SURVEY C-7); here the
 * original volume is passed explicitly.  n = number of voxels.
 * Alignment: decoded_dev, original_dev and error_dev at any byte offset, each independently; vr_query_error writes
 * exactly n bytes. */
vr_status vr_measure_error(const uint8_t *decoded_dev, const uint8_t *original_dev, int64_t n,
                           int32_t *max_error, double *mean_error, void *stream);
vr_status vr_query_error(const uint8_t *decoded_dev, const uint8_t *original_dev, int64_t n,
                         uint8_t *error_dev, void *stream);

/* ---- error-bounded level of detail (new): what every cut of every brick costs in accuracy, and the cuts a bound allows
 * The error of brick b between two buffers of num_bricks bricks x V bytes (brick b at byte b * V of each) is four exact
 * integers over its V byte pairs (a, r): */
typedef struct vr_brick_error {
    uint64_t sum_abs;   /* sum |a-r|            */
    uint64_t sum_sq;    /* sum (a-r)^2          */
    uint32_t max_abs;   /* max |a-r|            */
    uint32_t num_diff;  /* voxels with a != r   */
} vr_brick_error;       /* 24 bytes */

/* The rule of the three calls below:
 *  - the ERROR TABLE of a set for the cuts cut_lo .. cut_hi against a reference (the original voxels, or any decode, in
 *    vr_brickset_build's layout) has one row per cut: entry (c - cut_lo) * B + b is the error between brick b of
 *    vr_brickset_decode(bs, c, ...) and brick b of the reference.  The decodes are the set's own uniform decodes, the same
 *    bytes, into the caller's scratch; each is followed by one reduction kernel.  Every field is exact and independent of
 *    the launch shape: only integer adds and maxima cross lanes, waves and workgroups.  Against the set's own full-depth
 *    decode the row of cut max_tree_depth is all zero.
 *  - the SELECTION: for brick b, h = cuts_in ? cuts_in[b] : cut_hi.  h == -1 stays -1 (a culled brick).  Otherwise the
 *    candidates are the cuts c in [cut_lo, min(h, cut_hi)]; c qualifies iff max_abs <= max_abs_bound and, when
 *    mean_sq_bound >= 0, (double)sum_sq <= mean_sq_bound * (double)voxels_per_brick (one double multiply, one comparison);
 *    cuts_out[b] = the smallest qualifying candidate, or h if there is none (also when h < cut_lo).  Error need not fall
 *    with the cut and the rule does not assume it.  cuts_in is what vr_lod_select returns: geometry first, then data.
 *    Bound 0 against the set's full-depth decode gives cuts whose vr_brickset_decode_lod output equals the full decode bit
 *    for bit, in fewer pool bytes and less decode work.
 * vr_measure_error_bricks is the reduction on its own, for any two device buffers.  VR_ERR_INVALID for a null pointer,
 * num_bricks < 1 or voxels_per_brick outside 1 .. 2^32 - 1 (inside it num_diff is exact and sum_sq below 2^48); then
 * VR_ERR_NO_DEVICE.  It synchronises `stream` before it returns.
 * vr_brickset_error_table: scratch_dev holds num_bricks * X*Y*Z bytes and is left with the decode at cut_hi; table_host
 * receives (cut_hi - cut_lo + 1) * num_bricks entries.  All cuts are queued on `stream` with no host synchronisation in
 * between (a set opened from a file fills the cut values of a cut above its index level on the host, as
 * vr_brickset_decode does: such a cut waits for the stream first); one download and one synchronisation end the call.
 * The device table belongs to the set: allocated on first use, cleared on the stream, freed by vr_brickset_destroy.
 * Every variant, and sets opened from a file.  VR_ERR_INVALID (nothing launched) for a null pointer, cut_lo < 0,
 * cut_hi > max_tree_depth, cut_lo > cut_hi, or a scratch_dev that vr_brickset_decode would refuse at one of the cuts;
 * VR_ERR_STATE before build.
 * vr_lod_select_error is host-only (no device needed).  VR_ERR_INVALID for a null table or cuts_out, num_bricks < 1,
 * cut_lo < 0, cut_lo > cut_hi, voxels_per_brick < 1, max_abs_bound < 0, a NaN mean_sq_bound, or a cuts_in[b] < -1
 * (cuts_out is then not written).
 * Alignment: decoded_dev, reference_dev at any byte offset, each independently (16-byte loads where a brick starts at the
 * same offset modulo 16 in both, single bytes otherwise); scratch_dev as vr_brickset_decode's out_dev. */
vr_status vr_measure_error_bricks(const uint8_t *decoded_dev, const uint8_t *reference_dev, int32_t num_bricks,
                                  int64_t voxels_per_brick, vr_brick_error *out_host, void *stream);
vr_status vr_brickset_error_table(vr_brickset *bs, const uint8_t *reference_dev, uint8_t *scratch_dev, int32_t cut_lo,
                                  int32_t cut_hi, vr_brick_error *table_host, void *stream);
vr_status vr_lod_select_error(const vr_brick_error *table, int32_t num_bricks, int32_t cut_lo, int32_t cut_hi,
                              int64_t voxels_per_brick, const int32_t *cuts_in, int32_t max_abs_bound, double mean_sq_bound,
                              int32_t *cuts_out);

/* ---- volume histograms (new): what values a volume holds -- per brick, of a pool, and by value and gradient ------------
 * Every count is an exact integer, and counts add: the tables of parts of a volume (bricks, cells, the own boxes of
 * several GPUs) sum to the table of the whole with no tolerance.  No result depends on the launch shape.
 *
 * vr_histogram_bricks: vr_measure_error_bricks' layout, brick b at byte b * V of data_dev, which may start at any byte
 * (bytes up to the next 16-byte boundary one by one, aligned 16-byte loads, the last bytes one by one).
 * bricks_host[b * 256 + k] = the number of bytes of brick b that equal k; total_host[k] = the sum over the bricks,
 * carried in 64 bits on the device as well.  Either output may be NULL.  V lies in 1 .. 2^32 - 1, so a per-brick count
 * fits 32 bits.  VR_ERR_INVALID for a null data_dev, both outputs null, num_bricks < 1 or V outside that range; then
 * VR_ERR_NO_DEVICE.  The device tables are the call's own: allocated, cleared on `stream`, downloaded, freed; the call
 * synchronises `stream` before it returns.
 *
 * vr_histogram_pool: the histogram of the virtual volume vr_raycast_pool reads, per grid cell (x fastest) and in total.
 * A cell with offset >= 0 counts every stored voxel 1 << (shift_x + shift_y + shift_z) times; an absent cell counts
 * X*Y*Z in bin 0, for the pool reads as 0 there, and its pool bytes are not touched.  Per cell and in total the result
 * equals vr_histogram_bricks of that volume laid out brick by brick.  The table is read on the device.  Restrictions:
 * vr_raycast_pool's (power-of-two brick_dims, virtual extents below 2^31), X*Y*Z <= 2^32 - 1 and fewer than 2^31 cells;
 * VR_ERR_INVALID otherwise, for a null pointer, or with both outputs null.  pool_dev at any byte; table_dev 16-byte
 * aligned, else VR_ERR_INVALID, nothing launched (the table contract, at vr_pool_entry).  Synchronises `stream`.
 *
 * vr_histogram2d: the joint histogram of value and gradient magnitude of a dense volume, the design space of a
 * two-dimensional transfer function.  volume_dev holds the voxels [vol_origin, vol_origin + dims) of a global volume of
 * G = global_dims voxels (a global_dims extent of 0 means dims' own).  For every OWNED voxel p, own_lo <= p < own_hi in
 * global coordinates: v = its value; d_x = v(p + e_x) - v(p - e_x), d_y and d_z likewise, every index clamped to
 * [0, G - 1] -- the integers the lit marcher interpolates (gradient-shaded rendering, above); s = d_x^2 + d_y^2 + d_z^2;
 * r = isqrt(s) >> 2 with isqrt the exact integer square root (a float sqrt corrected by one step either way); the voxel
 * counts in hist_host[r * 256 + v], a table of VR_HIST_GRAD_BINS x VR_HIST_BINS 64-bit counts.
 * VR_ERR_INVALID, nothing launched: a null pointer; dims or global_dims as vr_raycast refuses them; a local volume that
 * leaves the global one; and, per axis, an own box that is empty (own_lo >= own_hi), that leaves the local volume
 * (own_lo < vol_origin or own_hi > vol_origin + dims), or one of whose clamped neighbours would:
 * max(own_lo - 1, 0) < vol_origin or min(own_hi, G - 1) > vol_origin + dims - 1.  With that check the kernel cannot form
 * an address outside volume_dev.  A slab of several GPUs therefore holds ONE halo layer beyond its own box.  Invariants:
 * the column sums of the table are the 256-bin histogram of the owned voxels; the tables of disjoint own boxes that
 * tile the volume add up to the table of the whole volume.  volume_dev at any byte.  Synchronises `stream`.
 *
 * vr_window_from_histogram is host-only (no device needed): a display window from the percentiles of a 256-bin
 * histogram, for the window_lo / window_hi of a projection.  N = the sum of hist[k] over k >= first_bin (first_bin = 1
 * leaves the background out); cum_k = the sum of hist[first_bin .. k].  lo_k = the smallest k >= first_bin with
 * (double)cum_k > lo_fraction * (double)N, or, where there is none (lo_fraction = 1), the largest k with hist[k] != 0;
 * hi_k = the smallest k >= first_bin with (double)cum_k >= hi_fraction * (double)N.  If hi_k <= lo_k then hi_k = lo_k + 1,
 * and if that is 256 both move down by one.  *window_lo = (float)lo_k / 255.0f, *window_hi = (float)hi_k / 255.0f: always
 * 0 <= window_lo < window_hi <= 1, a window vr_raycast_projection accepts.  VR_ERR_INVALID for a null pointer, first_bin
 * outside 0 .. 255, a fraction outside [0, 1] or NaN, lo_fraction > hi_fraction, or N == 0. */
#define VR_HIST_BINS      256
#define VR_HIST_GRAD_BINS 111      /* isqrt(3 * 255^2) >> 2 = 110 */
vr_status vr_histogram_bricks(const uint8_t *data_dev, int32_t num_bricks, int64_t voxels_per_brick,
                              uint32_t *bricks_host /* B*256 or NULL */, uint64_t *total_host /* 256 or NULL */,
                              void *stream);
vr_status vr_histogram_pool(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                            const int64_t grid[3], uint32_t *cells_host /* cells*256 or NULL */,
                            uint64_t *total_host /* 256 or NULL */, void *stream);
vr_status vr_histogram2d(const uint8_t *volume_dev, const int64_t dims[3], const int64_t global_dims[3],
                         const int64_t vol_origin[3], const int64_t own_lo[3], const int64_t own_hi[3],
                         uint64_t *hist_host /* 111*256 */, void *stream);
vr_status vr_window_from_histogram(const uint64_t *hist /* 256 */, int32_t first_bin, double lo_fraction,
                                   double hi_fraction, float *window_lo, float *window_hi);

/* ---- iso-surface meshes (new): the surface itself, as indexed watertight triangles -------------------------------------
 * The mesh of the iso-surface of a dense volume, by one exact rule: counts and indices are integers, a vertex depends
 * on two voxels alone, and the meshes of disjoint cell boxes concatenate to the mesh of the whole.  Nothing below
 * depends on the launch shape; two calls on the same input write the same bytes.
 *
 * Lattice.  The lattice points are the voxel centres of the global volume of G = global_dims voxels (an extent of 0
 * means dims' own); v(q) is the voxel at q.  With cap == 0 the lattice is 0 .. G_k - 1 per axis.  With cap == 1 it is
 * -1 .. G_k, and v(q) = 0 wherever a coordinate is -1 or G_k: capping closes every surface at the volume's faces.
 *
 * Inside test.  level = iso_value * 255.0f, a float32 product (iso_value as in vr_render_params);
 * inside(q) = (float)v(q) >= level, the side the iso-surface marcher calls ">= iso".
 *
 * Cells.  A cell is the cube with low corner c; cells exist for 0 <= c_k <= G_k - 2 without cap and for
 * -1 <= c_k <= G_k - 1 with it.  Every cell is split into the six Kuhn tetrahedra around its main diagonal: for each
 * permutation pi of the axes in lexicographic order (xyz, xzy, yxz, yzx, zxy, zyx) the tetrahedron
 * a0 = c, a1 = a0 + e_pi1, a2 = a1 + e_pi2, a3 = c + (1,1,1).  The split is translation invariant, so neighbouring cells
 * agree on their shared faces: there are no ambiguous cases.
 *
 * Edge vertices.  A lattice edge is (p, d), d in {0,1}^3 \ 0, owned by its low endpoint p; its type is
 * e = d_x + 2 d_y + 4 d_z - 1, in 0 .. 6.  It carries a vertex iff inside(p) != inside(p + d).  The vertex is
 * pos_k = (float)p_k + (d_k ? t : 0.0f) with t = (level - (float)v(p)) / ((float)v(p + d) - (float)v(p)), one correctly
 * rounded float32 division.  Positions are in voxel-centre index coordinates: texture space is (pos + 0.5) / G, and the
 * renderer's world cube is that minus 0.5.
 *
 * Triangles of one tetrahedron.  m_i = inside(a_i); (i, j) with i < j names the edge (a_i, a_j - a_i).
 *   all four corners equal: no triangle;
 *   one corner i differs from the other three: one triangle with the corners (i, j), j != i ascending;
 *   two inside i < j and two outside k < l: the quad q = (i,k), (i,l), (j,l), (j,k) gives (q0,q1,q2) and (q0,q2,q3).
 * A triangle winds counter-clockwise seen from the outside (the lower-value side).  Where the order above winds the
 * other way the single triangle swaps its last two corners, and the quad becomes (q0,q3,q2), (q0,q2,q1).  The winding
 * depends on (pi, m) alone, not on t.
 *
 * Ownership and order.  The call owns the cells own_lo <= c < own_hi (global cell coordinates); a box that is empty on
 * some axis is allowed and gives an empty mesh.
 *   triangles: those of the owned cells, ordered by cell (x fastest), then tetrahedron, then the order above;
 *   vertices: every crossing edge whose two endpoints lie in the closed point box [own_lo, own_hi] -- exactly the edges
 *     of the owned cells -- ordered by owner point (x fastest over that point box), then type e.  Indices are uint32
 *     into this list: a vertex shared by up to six triangles is stored once.
 *
 * Gradients (optional).  One float3 per vertex, g = ga + t * (gb - ga) per component in that operation order, ga and gb
 * the integer central differences v^(q + e_k) - v^(q - e_k) at the edge's two endpoints; v^ = v with the indices clamped
 * to [0, G - 1] when cap == 0, zero-extended outside the volume when cap == 1.  The same integers as the lit marcher's
 * and the joint histogram's.  Unnormalised and exact; -g is the outward normal.
 *
 * Workspace.  N = the number of points of the own point box, the product of own_hi_k - own_lo_k + 1 (0 for a box empty
 * on some axis); R = ceil(N / 64) runs of 64 points; B = ceil(R / 1024).  With up16 rounding up to a multiple of 16,
 *   bytes = up16(2 N) + 2 up16(4 R) + 16 B + 16:
 * per point a 16-bit word (the 7-bit mask of its crossing edges and the 9-bit count of the vertices before it in its
 * run), per run a 32-bit first vertex and first triangle, per 1024 runs two 64-bit sums, and the two totals.  About
 * 2.13 bytes per point.  workspace_dev must be 16-byte aligned.
 *
 * vr_isomesh_workspace_bytes is host-only.  vr_isomesh_count fills the workspace and reports {vertices, triangles} as
 * 64-bit counts; it synchronises `stream`.  More than VR_ISOMESH_MAX_VERTICES vertices or VR_ISOMESH_MAX_TRIANGLES
 * triangles: VR_ERR_UNSUPPORTED, with the counts still reported.  A box of more than 2^36 points: VR_ERR_UNSUPPORTED.
 * vr_isomesh_emit takes the same volume and desc as the count, and the counts it reported: positions_dev 3 floats per
 * vertex, gradients_dev likewise or NULL, indices_dev 3 uint32 per triangle; asynchronous on `stream`.  Every store is
 * guarded by the two counts passed in: a stale or foreign workspace can produce a wrong mesh, never a write outside
 * the three outputs.  The three outputs may be 4-byte aligned; volume_dev may start at any byte.  Zero counts launch
 * nothing and return VR_OK; positions_dev may be NULL where num_vertices is 0, indices_dev where num_triangles is 0.
 *
 * VR_ERR_INVALID, nothing launched, before VR_ERR_NO_DEVICE: a null pointer; a workspace that is not 16-byte or an
 * output that is not 4-byte aligned; dims or global_dims as vr_raycast refuses them; a local volume that leaves the
 * global one; cap not 0 or 1; iso_value not finite; per axis an own box outside the cell range of its cap setting
 * (own_lo < 0 or own_hi > G - 1 without cap, own_lo < -1 or own_hi > G with it) or with own_lo > own_hi; a held volume
 * that does not contain every in-volume point of [own_lo, own_hi]: max(own_lo, 0) < vol_origin or
 * min(own_hi, G - 1) > vol_origin + dims - 1; with gradients_dev, the same with the box grown by one point on both
 * sides; counts that are negative or beyond the two limits.  With these checks no kernel can form an address outside
 * volume_dev.  A slab of several GPUs holds the points of its own box, and one layer more for gradients; the ranks'
 * meshes concatenate (seam vertices are stored by both neighbours, bit for bit equal). */
#define VR_ISOMESH_MAX_VERTICES  4294967295ull     /* 2^32 - 1 */
#define VR_ISOMESH_MAX_TRIANGLES 1431655765ull     /* 2^32 / 3 */
typedef struct vr_isomesh_desc {
    float   iso_value;
    int32_t cap;                /* 0 or 1 */
    int64_t global_dims[3];     /* 0 = dims */
    int64_t vol_origin[3];
    int64_t own_lo[3];          /* owned cells, global cell coordinates: own_lo <= c < own_hi */
    int64_t own_hi[3];
} vr_isomesh_desc;              /* 104 bytes */
vr_status vr_isomesh_workspace_bytes(const int64_t dims[3], const vr_isomesh_desc *desc, int64_t *bytes);
vr_status vr_isomesh_count(const uint8_t *volume_dev, const int64_t dims[3], const vr_isomesh_desc *desc,
                           void *workspace_dev, uint64_t counts_host[2], void *stream);
vr_status vr_isomesh_emit(const uint8_t *volume_dev, const int64_t dims[3], const vr_isomesh_desc *desc,
                          const void *workspace_dev, int64_t num_vertices, int64_t num_triangles, float *positions_dev,
                          float *gradients_dev /* or NULL */, uint32_t *indices_dev, void *stream);

/* ---- ingest: VolumeReader<T>::LoadBricksToTexture (VolumeReader.h:151-223) ------
 * Places brick b (brick_dims, x-fastest, contiguous at bricks_dev + b*brick_voxels)
 * at grid cell brick_ijk[3*b..3*b+2] of a global x-fastest volume of
 * (I*X, J*Y, K*Z) voxels: volume_dev must hold I*J*K*X*Y*Z bytes whatever num_bricks is (grid cells
 * without a brick are left untouched; the reference sizes its array by numBricks, VolumeReader.h:163-168,
 * and overruns it for sparse brick lists -- not reproduced).  64-bit indices (the reference's 32-bit ones wrap above
 * 2^32 voxels, VolumeReader.h:171).  vr_disassemble_bricks is the inverse (global
 * volume -> contiguous bricks), used to feed per-brick trees.  Either buffer may start at any byte (16-byte vector
 * copies where both are 16-byte aligned, byte copies otherwise: no reliance on the hardware's tolerance of misaligned
 * vector loads).  num_bricks above VR_MAX_BRICKS is VR_ERR_UNSUPPORTED, as for vr_brickset_create and for the same
 * reason, before the device is touched (a longer brick list goes in several calls). */
vr_status vr_assemble_bricks(const uint8_t *bricks_dev, int32_t num_bricks, const int64_t brick_dims[3],
                             const int64_t *brick_ijk, const int64_t grid[3], uint8_t *volume_dev, void *stream);
vr_status vr_disassemble_bricks(const uint8_t *volume_dev, int32_t num_bricks, const int64_t brick_dims[3],
                                const int64_t *brick_ijk, const int64_t grid[3], uint8_t *bricks_dev, void *stream);

/* ---- render: raycaster.frag / isosurface.frag on the UnitBrick proxy cube --------
 * Camera = the values main.cpp feeds glm::lookAt / glm::perspectiveFov (main.cpp:33-40,396-397). */
typedef struct vr_camera {
    float pos[3];      /* cameraPos   (0,0,-0.75)  */
    float front[3];    /* cameraFront (0,0,1)      */
    float up[3];       /* cameraUp    (0,1,0)      */
    float fov_deg;     /* fov 50                   */
    float z_near, z_far; /* 0.1, 100               */
} vr_camera;

enum { VR_RENDER_COMPOSITE = 0 /* raycaster.frag */, VR_RENDER_ISOSURFACE = 1 /* isosurface.frag */,
       VR_RENDER_PARTIAL = 2 /* raycaster.frag accumulation as an (rgb-premultiplied c, transmittance) pair for sort-last compositing */,
       VR_RENDER_SHADED = 3 /* transfer function with gradient lighting, or a two-dimensional one: vr_raycast_tf_shaded, vr_raycast_tf2d & co. only */,
       VR_RENDER_PROJECTION = 4 /* intensity projections: vr_raycast_projection & co. only */ };

typedef struct vr_render_params {
    int32_t width, height;   /* 1600x1200 in the reference (main.cpp:27); bench uses 1920x1080 */
    float step_size[3];      /* uniform step_size = 1/BRICK_DIM (main.cpp:330-331)             */
    float iso_value;         /* uniform isoValue = currIsoVal/255 (main.cpp:334)               */
    int32_t max_samples;     /* MAX_SAMPLES = 300 (raycaster.frag:14)                          */
    int32_t mode;            /* VR_RENDER_*                                                    */
    /* Sort-last multi-GPU path (VR_RENDER_PARTIAL): the rank owns the samples whose texture-space
     * position lies in [box_min, box_max); volume_dev holds the voxels [vol_origin, vol_origin+dims)
     * of a global volume of global_dims voxels (own slab plus halo layers for filtering).
     * Single-GPU path: box {0,0,0}-{1,1,1}, global_dims {0,0,0} (= dims), vol_origin {0,0,0}. */
    float box_min[3], box_max[3];
    int64_t global_dims[3];
    int64_t vol_origin[3];
    int32_t no_early_exit;   /* 1: ignore the alpha>0.99 exit (reference for the sort-last path)   */
    /* Empty-space skipping (new; the reference only hints at it, isosurface_compressed.frag:23-29): skip_grid_dev = a
     * grid built by vr_skip_grid_build from THE SAME volume_dev, skip_cell its cell size in voxels; NULL / 0 = off.
     * A sample whose eight taps are provably all zero (compositor) or provably all on one side of the iso value is not
     * fetched; the ray still advances sample by sample, so the frame is bit-identical to the one without the grid. */
    int32_t skip_cell;
    const uint8_t *skip_grid_dev;
} vr_render_params;

/* volume_dev: X*Y*Z uint8 (the 3-D texture contents, GL_RED/GL_UNSIGNED_BYTE, GL_LINEAR,
 * clamp-to-edge: VolumeReader.h:114-127).  rgba_dev: height*width*4 float32, row 0 = top.
 * Pixels not covered by the cube are white (main.cpp:392).  VR_ERR_INVALID (nothing launched) for any dims[k] <= 0 or
 * >= 2^31, width or height <= 0, max_samples < 0 or an unknown mode.  volume_dev and skip_grid_dev may start at any
 * byte. */
vr_status vr_raycast(const uint8_t *volume_dev, const int64_t dims[3], const vr_camera *cam,
                     const vr_render_params *params, float *rgba_dev, void *stream);

/* Host-only (no device needed): choose cuts_out[b] for vr_brickset_decode_lod, for the bricks of a volume laid out
 * as in vr_assemble_bricks (brick b at grid cell brick_ijk[3b..3b+2] of `grid`, each brick_dims voxels) and the frame
 * vr_raycast draws with (cam, params).  pixel_tolerance > 0.  The rule:
 *  - the volume is vr_raycast's unit cube: texture space [0,1]^3 = world [-0.5,0.5]^3, voxel size 1/G per axis,
 *    G = grid * brick_dims (params->global_dims where non-zero).  Brick b covers [ijk*brick_dims, (ijk+1)*brick_dims)/G.
 *  - its box is grown on every side by one voxel (the reach of a trilinear tap); in VR_RENDER_ISOSURFACE mode also by
 *    0.01 + max|step_size| (the gradient's offset, and the second fetch / bisection points that may leave the cube
 *    and read its clamped edge); in VR_RENDER_SHADED mode by two voxels instead of one (a lattice gradient's tap
 *    reaches one voxel beyond the trilinear taps).
 *  - culled (-1): the grown box lies wholly outside [box_min, box_max) on some axis, or all eight of its corners lie
 *    outside one plane of the frame's frustum.  The frustum is vr_raycast's: f = normalize(front),
 *    s = normalize(f x up), u = s x f, tanY = tan(fov/2), tanX = tanY * width / height (float, as vr_raycast); for a
 *    point p with d = p - pos, z = d.f, x = d.s, y = d.u the planes are z >= z_near, |x| <= tanX z, |y| <= tanY z and
 *    z <= z_far + (max_samples + 1) * max|step_size| (a ray enters the cube at depth <= z_far and marches on from
 *    there).  Each test allows 1e-6 * (1 + |z|) for rounding.  If f is parallel to up (s = 0) the side planes are
 *    not used.  No ray of the frame takes a sample or a tap from a culled brick.
 *  - projected voxel size s = (height / 2 / tanY) * max_k(1/G_k) / max(dist, z_near), dist = distance from pos to
 *    the grown box (0 inside it).
 *  - levels dropped k = 0 if s >= pixel_tolerance, else min(orig_tree_depth, floor(3 log2(pixel_tolerance / s)))
 *    (three tree levels halve the resolution on all three axes).
 *  - cut = max_tree_depth if k == 0 (the grown-branch levels refine values, not space: kept only when no spatial
 *    level is dropped), else orig_tree_depth - k. */
vr_status vr_lod_select(const vr_camera *cam, const vr_render_params *params, int32_t num_bricks,
                        const int64_t brick_dims[3], const int64_t *brick_ijk, const int64_t grid[3],
                        int32_t orig_tree_depth, int32_t max_tree_depth, float pixel_tolerance, int32_t *cuts_out);

/* (min, max) of every skip_cell^3 cell of the volume, widened by the one voxel a trilinear fetch reaches beyond its
 * base voxel: grid_dev holds 2 bytes per cell, cells x fastest, ceil(dims / skip_cell) cells per axis.  Exact bounds of
 * the DECODED voxels: MidRangeTree's half-range stream would give bounds of the original data one level above, but the
 * decoded scalar of an internal node is a prediction with no error bound, so mid +- range at a coarse cut is not a safe
 * bracket (vr_brickset_decode_range remains available for previews).  Both buffers may start at any byte. */
vr_status vr_skip_grid_build(const uint8_t *volume_dev, const int64_t dims[3], int32_t skip_cell, uint8_t *grid_dev,
                             void *stream);

/* vr_raycast and vr_skip_grid_build over a pool (vr_brickset_decode_lod_pool) in place of a dense volume.  The volume
 * is the virtual grid * brick_dims voxels whose voxel (x, y, z) is pool[e.offset + (lx >> sx) + (X >> sx) * ((ly >> sy)
 * + (Y >> sy) * (lz >> sz))], e = table_dev[cell], cell = (x / X, y / Y, z / Z), (lx, ly, lz) = the position in the
 * brick, and 0 where e.offset = -1.  Bit-identical to vr_raycast / vr_skip_grid_build on that volume assembled densely,
 * in every mode, with or without a skip grid (one built by vr_skip_grid_build_pool from the same pool and table, or by
 * vr_skip_grid_build from the dense volume: they are byte-identical).  brick_dims must be powers of two and the
 * virtual extents below 2^31; params->vol_origin must be 0 and params->global_dims 0 or the virtual extents, else
 * VR_ERR_INVALID.  table_dev 16-byte aligned, else VR_ERR_INVALID, nothing launched -- here and in every vr_raycast_pool_*
 * call below (the table contract, at vr_pool_entry); pool_dev at any byte. */
vr_status vr_raycast_pool(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                          const int64_t grid[3], const vr_camera *cam, const vr_render_params *params, float *rgba_dev,
                          void *stream);
vr_status vr_skip_grid_build_pool(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                                  const int64_t grid[3], int32_t skip_cell, uint8_t *grid_dev, void *stream);

/* ---- direct volume rendering with a user transfer function (new; the reference's compositor is hard-wired) --------
 * A transfer function is 256 entries of (r, g, b, a) float32, each in [0, 1]; entry k belongs to the scalar k / 255.
 * Ray set-up is vr_raycast's, unchanged: the pixel ray, the cube entry, vUV, gd, st = gd * step_size, pos += st, the
 * inside() stop and max_samples.  Each sample, in order:
 *  1. clip box: a pos outside [box_min, box_max) on any axis contributes nothing (the partial mode's ownership test;
 *     the single-GPU default {0,0,0}-{1,1,1} clips nothing);
 *  2. fetch: s = vr_raycast's trilinear sample, bit for bit (dense volume or pool);
 *  3. lookup: x = clamp(s * 255, 0, 255), i = min((int)x, 254), f = x - i; per channel e = lut[i] + f (lut[i+1] - lut[i]);
 *     e.a is clamped to [0, 1] against rounding;
 *  4. opacity correction: opacity_unit > 0: a = 1 - (1 - e.a)^(L / opacity_unit), L = |st| in texture space (fixed per
 *     ray); opacity_unit == 0: a = e.a.  e.a == 0 gives exactly 0; e.a == 1 with L > 0 gives exactly 1; L == 0 gives 0;
 *  5. over: C += (T a) e.rgb, then T *= 1 - a, from C = 0, T = 1;
 *  6. early exit once T < 0.01, unless no_early_exit (the mirror of raycaster.frag's A > 0.99).
 * The pixel is (C + T * background, 1 - T); a pixel the cube does not cover is (background, 0), the same value a
 * covered ray that gathers nothing produces.
 * From vr_render_params: width, height, step_size, max_samples, no_early_exit, box_min / box_max, global_dims,
 * vol_origin, skip_cell, skip_grid_dev (iso_value is ignored); mode must be VR_RENDER_COMPOSITE.  The skip grid has
 * vr_raycast's limit (used only where volume_dev is the whole volume).  A sample whose grid bounds are (mn, mx) is not
 * fetched when every entry in [max(mn - 1, 0), min(mx + 1, 255)] has alpha exactly 0 (the one-entry margin covers the
 * rounding of s * 255 past a tap's value): its a would be 0 and both updates of step 5 exact no-ops, so frames are
 * bit-identical with and without the grid. */
typedef struct vr_transfer_function {
    const float *lut_dev;     /* 256 x (r,g,b,a) float32 on the device, 16-byte aligned, values in [0,1] */
    float opacity_unit;       /* texture-space distance the alphas are defined for; 0 = no correction */
    float background[3];      /* colour behind the volume; (1,1,1) = the clear colour of main.cpp:392 */
} vr_transfer_function;       /* 24 bytes */

/* vr_raycast's checks, plus VR_ERR_INVALID (nothing launched) for a null tf or lut_dev, a lut_dev that is not 16-byte
 * aligned, an opacity_unit that is negative or not finite, a background that is not finite, or a mode other than
 * VR_RENDER_COMPOSITE.  The pool variant also takes vr_raycast_pool's restrictions and is bit-identical to
 * vr_raycast_tf of the pool's volume assembled densely. */
vr_status vr_raycast_tf(const uint8_t *volume_dev, const int64_t dims[3], const vr_camera *cam,
                        const vr_render_params *params, const vr_transfer_function *tf, float *rgba_dev, void *stream);
vr_status vr_raycast_pool_tf(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                             const int64_t grid[3], const vr_camera *cam, const vr_render_params *params,
                             const vr_transfer_function *tf, float *rgba_dev, void *stream);

/* ---- gradient-shaded direct volume rendering (new) -----------------------------------------------------------------
 * vr_raycast_tf's rule, steps 1-6 unchanged, except that step 5 adds (T a) c, a lit colour c in place of e.rgb, for
 * every sample whose a > 0 (a sample with a == 0 changes nothing, lit or not):
 *  - gradient on the lattice: (x0, y0, z0) = the sample's base voxel floor(pos * G - 0.5) and (fx, fy, fz) its weights,
 *    exactly as the trilinear fetch forms them; v(x, y, z) = the voxel at (x, y, z) with every index clamped to
 *    [0, G - 1] of the global volume (clamp-to-edge, as the fetch).  For each of the eight corners (x0+i, y0+j, z0+k),
 *    i, j, k in {0, 1}: d_x = v(x0+i+1, y0+j, z0+k) - v(x0+i-1, y0+j, z0+k), d_y and d_z likewise (integers).  The
 *    gradient g = the trilinear interpolation of d with the sample's weights, in the fetch's order, times 1 / (2 * 255);
 *  - m = |g| (grey levels per voxel / 255).  m <= grad_min: c = e.rgb (unlit).  Otherwise:
 *    N = normalize(G_x g_x, G_y g_y, G_z g_z) (the world-space normal of the unit cube, G the global extents);
 *    V = -gd (gd the normalized ray direction); L = normalize(light_dir), or V when light_dir is {0,0,0} (head light);
 *    H = normalize(L + V), and the specular term is 0 when L + V = 0;  two-sided: cd = |N.L|, ch = clamp(|N.H|, 1e-5, 1)
 *    (the iso-surface shader's 1e-5; the upper clamp only catches rounding);
 *    c = min(1, e.rgb (ambient + diffuse cd) + specular ch^shininess) per channel.
 * Alpha, opacity correction, the early exit, the skip grid and the pixel formula are vr_raycast_tf's.  Invariants:
 *  - ambient = 1, diffuse = specular = 0 gives frames bit-identical to vr_raycast_tf in VR_RENDER_COMPOSITE mode with
 *    the same params: e.rgb is formed by the same expression, e.rgb * 1 + 0 is exact, and the min(1, .) is a no-op
 *    because e = lut[i] + f (lut[i+1] - lut[i]) never rounds above 1 for table values in [0, 1];
 *  - frames are bit-identical with and without the skip grid: the grid's decision depends on alpha alone;
 *  - the pool frame is bit-identical to the dense frame of the pool's volume assembled densely;
 *  - a slab under vol_origin / global_dims must hold TWO halo layers (the gradient reaches one voxel beyond the taps)
 *    to equal the full volume inside its box. */
typedef struct vr_shading {
    float ambient, diffuse, specular, shininess;  /* ka, kd, ks >= 0; shininess >= 0; all finite */
    float light_dir[3];   /* world direction towards the light; {0,0,0} = head light (L = V) */
    float grad_min;       /* >= 0: samples whose gradient magnitude is <= grad_min are not lit */
} vr_shading;             /* 32 bytes */

/* vr_raycast_tf's / vr_raycast_pool_tf's checks, except that params->mode must be VR_RENDER_SHADED, plus VR_ERR_INVALID
 * (nothing launched) for a null shading or any of its fields negative (light_dir excepted) or not finite.  The pool
 * variant is bit-identical to vr_raycast_tf_shaded of the pool's volume assembled densely. */
vr_status vr_raycast_tf_shaded(const uint8_t *volume_dev, const int64_t dims[3], const vr_camera *cam,
                               const vr_render_params *params, const vr_transfer_function *tf, const vr_shading *shading,
                               float *rgba_dev, void *stream);
vr_status vr_raycast_pool_tf_shaded(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                                    const int64_t grid[3], const vr_camera *cam, const vr_render_params *params,
                                    const vr_transfer_function *tf, const vr_shading *shading, float *rgba_dev,
                                    void *stream);

/* ---- sort-last colour partials (new): frames through a transfer function, lit or not, drawn by several GPUs ----------
 * A colour partial is one float4 per pixel, (C.r, C.g, C.b, T): the premultiplied colour and the transmittance of
 * vr_raycast_tf's rule when its loop ends (steps 1-6 unchanged; the early exit of step 6 is local to the rank), stored as
 * they are instead of (C + T * background, 1 - T).  A pixel the cube does not cover, or whose ray owns no sample in
 * [box_min, box_max), is (0, 0, 0, 1) exactly; there is no coverage flag, because finishing (0, 0, 0, 1) gives
 * (background, 0), the pixel vr_raycast_tf writes there.
 * shading == NULL: the unlit march, params->mode must be VR_RENDER_COMPOSITE and the checks are vr_raycast_tf's; with a
 * shading: the lit march, mode must be VR_RENDER_SHADED and the checks are vr_raycast_tf_shaded's (the pool variants:
 * those of vr_raycast_pool_tf / vr_raycast_pool_tf_shaded).  tf->background is validated but not used.  A rank's slab
 * under vol_origin / global_dims holds ONE halo layer unlit and TWO lit (see vr_shading).  Guarantees: a full-box partial
 * finished by vr_composite_finish_tf (or vr_composite_slabs_tf with one slab) equals the frame of vr_raycast_tf /
 * vr_raycast_tf_shaded bit for bit; the partial is bit-identical with and without the skip grid; the pool partial is
 * bit-identical to the dense partial of the pool's volume assembled densely. */
vr_status vr_raycast_tf_partial(const uint8_t *volume_dev, const int64_t dims[3], const vr_camera *cam,
                                const vr_render_params *params, const vr_transfer_function *tf,
                                const vr_shading *shading /* NULL = unlit */, float *partial_dev, void *stream);
vr_status vr_raycast_pool_tf_partial(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                                     const int64_t grid[3], const vr_camera *cam, const vr_render_params *params,
                                     const vr_transfer_function *tf, const vr_shading *shading /* NULL = unlit */,
                                     float *partial_dev, void *stream);
/* Combining colour partials.  over: front = front OVER back on all four floats, (C1 + T1*C2, T1*T2).  finish:
 * (C + T * background, 1 - T), the marcher's final store.  slabs: vr_composite_slabs for colour -- every pixel walks the
 * num_slabs partials of its tile in ITS view order (the sign of the pixel ray's component along `axis`, formed exactly
 * as vr_composite_slabs forms it), accumulates C += T * C_k, T *= T_k from C = 0, T = 1 and finishes.  The three are
 * written with the same operations in the same order: folding slabs pairwise in view order and finishing equals the
 * slab call bit for bit.  Of tf only background is read: a null lut_dev is allowed here.  VR_ERR_INVALID for a null
 * pointer, num_pixels < 1, num_slabs < 1, axis outside 0..2, a tile that leaves the frame or a background that is not
 * finite. */
vr_status vr_composite_over_tf(float *front_dev, const float *back_dev, int64_t num_pixels, void *stream);
vr_status vr_composite_finish_tf(const float *partial_dev, const vr_transfer_function *tf, float *rgba_dev,
                                 int64_t num_pixels, void *stream);
vr_status vr_composite_slabs_tf(const float *partials_dev, int32_t num_slabs, int64_t num_pixels, int64_t first_pixel,
                                int32_t axis, const vr_camera *cam, const vr_render_params *params,
                                const vr_transfer_function *tf, float *rgba_dev, void *stream);

/* ---- two-dimensional transfer functions (new): colour and opacity by value AND gradient magnitude --------------------
 * The table is rows x 256 entries of (r, g, b, a) float32, row-major, values in [0, 1]: entry [j][k] belongs to the scalar
 * k / 255 and the gradient coordinate j.  2 <= rows <= VR_TF2D_MAX_ROWS.  Ray set-up and steps 1, 2, 4, 5, 6 of
 * vr_raycast_tf's rule are unchanged; step 3 becomes:
 *  - x, i, f exactly as vr_raycast_tf forms them;
 *  - g = the lattice gradient of the sample exactly as vr_raycast_tf_shaded forms it, for EVERY fetched sample (not only
 *    those with a > 0), and m = sqrtf(g0*g0 + g1*g1 + g2*g2), the lit path's expression;
 *  - y = fminf(fmaxf(m * grad_scale, 0), (float)(rows - 1)); j = min((int)y, rows - 2); h = y - (float)j;
 *  - per channel eA = lut[j][i] + f * (lut[j][i+1] - lut[j][i]), eB likewise from row j + 1, e = eA + h * (eB - eA);
 *    e.a is clamped to [0, 1].
 * With grad_scale = 127.5 and rows = VR_HIST_GRAD_BINS, y = |d| / 4 (d the integer central differences): the row axis of
 * vr_histogram2d -- at a voxel centre floor(y) is that voxel's histogram row.
 * With a shading the lit colour c is formed from e.rgb and the same g and m by vr_raycast_tf_shaded's rule; with
 * shading == NULL, c = e.rgb.  params->mode must be VR_RENDER_SHADED in BOTH cases: the mode tells vr_lod_select that taps
 * reach two voxels.  A slab under vol_origin / global_dims holds TWO halo layers, lit or not.
 * Skip grid: columns[k] = the first j >= k at which ANY row has alpha != 0 at entry j, or 256 (vr_tf2d_columns_build).  A
 * sample whose grid bounds are (mn, mx) is not fetched when columns[max(mn - 1, 0)] > min(mx + 1, 255): then eA.a = eB.a
 * = 0, e.a = 0 + h * 0 = 0 exactly and both updates are exact no-ops, so frames are bit-identical with and without the
 * grid.  A skip grid attached (skip_grid_dev non-null and skip_cell > 0) with columns_dev == NULL is VR_ERR_INVALID.
 * Invariants:
 *  - a table whose rows are all equal draws vr_raycast_tf's frame with shading NULL, vr_raycast_tf_shaded's with a
 *    shading and vr_raycast_tf_partial's partials bit for bit (params differing in the mode only), for any grad_scale:
 *    eB - eA is exactly 0 and the build has no FMA contraction;
 *  - the pool call equals the dense call on the pool's volume assembled densely;
 *  - a full-box partial finished by vr_composite_finish_tf equals the frame.  Partials are colour partials: they go
 *    through vr_composite_over_tf / _finish_tf / _slabs_tf and vr_compositor_composite_tf unchanged, with a
 *    vr_transfer_function that carries the background. */
#define VR_TF2D_MAX_ROWS 256       /* 256 x 256 x 16 bytes = 1 MiB */
typedef struct vr_transfer_function2d {
    const float    *lut_dev;      /* rows x 256 x (r,g,b,a), 16-byte aligned */
    const uint16_t *columns_dev;  /* 256 x uint16 from vr_tf2d_columns_build of THE SAME table, 16-byte aligned; may be NULL when no skip grid is attached */
    int32_t rows;
    float   grad_scale;           /* > 0, finite: row coordinate y = m * grad_scale */
    float   opacity_unit;         /* as vr_transfer_function */
    float   background[3];
} vr_transfer_function2d;         /* 40 bytes */

/* columns_dev[k] for k = 0..255 (see above).  VR_ERR_INVALID for a null or misaligned lut_dev or columns_dev or rows out
 * of range. */
vr_status vr_tf2d_columns_build(const float *lut_dev, int32_t rows, uint16_t *columns_dev, void *stream);

/* The checks of vr_raycast_tf_shaded / vr_raycast_pool_tf_shaded (shading may be NULL = unlit; a shading given is
 * checked), plus VR_ERR_INVALID (nothing launched) for a null or misaligned lut_dev, a misaligned columns_dev, rows out
 * of range, a grad_scale that is not finite or <= 0, the missing-columns case above, or a mode other than
 * VR_RENDER_SHADED.  Then VR_ERR_NO_DEVICE.  The _partial calls write the colour partial (C.r, C.g, C.b, T). */
vr_status vr_raycast_tf2d(const uint8_t *volume_dev, const int64_t dims[3], const vr_camera *cam,
                          const vr_render_params *params, const vr_transfer_function2d *tf,
                          const vr_shading *shading /* NULL = unlit */, float *rgba_dev, void *stream);
vr_status vr_raycast_pool_tf2d(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                               const int64_t grid[3], const vr_camera *cam, const vr_render_params *params,
                               const vr_transfer_function2d *tf, const vr_shading *shading /* NULL = unlit */,
                               float *rgba_dev, void *stream);
vr_status vr_raycast_tf2d_partial(const uint8_t *volume_dev, const int64_t dims[3], const vr_camera *cam,
                                  const vr_render_params *params, const vr_transfer_function2d *tf,
                                  const vr_shading *shading /* NULL = unlit */, float *partial_dev, void *stream);
vr_status vr_raycast_pool_tf2d_partial(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                                       const int64_t grid[3], const vr_camera *cam, const vr_render_params *params,
                                       const vr_transfer_function2d *tf, const vr_shading *shading /* NULL = unlit */,
                                       float *partial_dev, void *stream);

/* ---- intensity projections (new): MIP, MinIP and the mean along the ray, exact across GPUs ----------------------------
 * Ray set-up is vr_raycast's, unchanged: positions are formed by the same repeated float additions pos += st, with the
 * same inside() stop and max_samples.  A sample is OWNED when its position lies in [box_min, box_max) on every axis
 * (vr_raycast_tf's step 1); an owned sample is fetched exactly as vr_raycast fetches it, bit for bit (dense volume or
 * pool).  The ray keeps n, the number of owned samples, and v:
 *   VR_PROJECT_MAX   v = the largest sample (a running maximum that starts at 0: samples are never negative);
 *   VR_PROJECT_MIN   v = the smallest sample (a running minimum that starts at +inf);
 *   VR_PROJECT_MEAN  v = the float32 sum of the samples, accumulated in sample order.
 * There is no early exit: no_early_exit and iso_value are ignored.
 * The projection PARTIAL is one float4 per pixel, (v, (float)n, 0, 0); a pixel the cube does not cover, or whose ray owns
 * no sample, is (0, 0, 0, 0) exactly.  max_samples above 2^24 is VR_ERR_INVALID, so that n is exact in a float.
 * The FINISH (partial to pixel): n == 0: (background, 0).  Otherwise m = v (MAX, MIN) or v / n (MEAN, a float32
 * division); w = clamp((m - window_lo) / (window_hi - window_lo), 0, 1); lut_dev == NULL: the pixel is (w, w, w, 1); else
 * e = step 3 of vr_raycast_tf's rule applied to w (the lookup, alpha clamped) and the pixel is
 * (e.a * e.rgb + (1 - e.a) * background, e.a).  With the window (0, 1), w == m exactly: (m - 0) / 1 is exact and m lies in
 * [0, 1].
 * The COMBINE of partials: partials with n == 0 are ignored; n adds; v is the max, the min, or the float32 sum in
 * ascending slab index.  Max, min and a count are commutative and associative, so the MAX and MIN frames (and partials)
 * of any number of ranks along any slab axis, combined in any order, equal the single-GPU frame bit for bit; MEAN's n is
 * exact and its v differs by the rounding of two summation orders.  A rank's slab under vol_origin / global_dims holds
 * ONE halo layer.
 * The skip grid (same condition as vr_raycast: volume_dev is the whole volume, or a pool's grid): the ray still advances
 * sample by sample and n still counts the sample; only the fetch is dropped.  With (mn, mx) the cell's bounds, k = 1/255
 * and cur the running value:
 *   MAX   skip iff (mn == mx ? (float)mx * k : (float)(mx + 1) * k) <= cur.  Equal bounds: all eight taps are equal, every
 *         c + f * (c - c) is exactly c, so the sample is exactly (float)mx * k and max(cur, sample) == cur.  Otherwise
 *         interpolation can leave the taps' range by rounding only, and a whole grey level covers that (the iso-surface's
 *         convention);
 *   MIN   skip iff (mn == mx ? (float)mn * k : (float)(mn - 1) * k) >= cur; never for the first owned sample (cur = +inf);
 *   MEAN  skip iff mx == 0: the sample is exactly 0 and sum + 0 is a no-op.
 * Frames and partials are bit-identical with and without the grid, and the pool's to the dense ones of the pool's volume
 * assembled densely.  finish(partial) equals the frame bit for bit, and pairwise vr_composite_combine_proj folds in
 * ascending order followed by the finish equal vr_composite_slabs_proj bit for bit (one combine and one finish are shared
 * by all of them). */
enum { VR_PROJECT_MAX = 0, VR_PROJECT_MIN = 1, VR_PROJECT_MEAN = 2 };

typedef struct vr_projection {
    const float *lut_dev;    /* NULL = grey; else 256 x (r,g,b,a) float32 on the device, 16-byte aligned (a colour map) */
    int32_t op;              /* VR_PROJECT_*  */
    float window_lo, window_hi;   /* the displayed value is clamp((m - lo) / (hi - lo), 0, 1); 0, 1 = identity */
    float background[3];
} vr_projection;             /* 32 bytes */

/* vr_raycast's / vr_raycast_pool's checks, plus VR_ERR_INVALID (nothing launched) for a mode other than
 * VR_RENDER_PROJECTION, a null proj, an op outside 0..2, a window that is not finite or has hi <= lo, a background that is
 * not finite, a lut_dev that is neither NULL nor 16-byte aligned, or max_samples > 2^24.  The _partial calls write the
 * partial instead of the frame: lut_dev, window and background are validated, not used. */
vr_status vr_raycast_projection(const uint8_t *volume_dev, const int64_t dims[3], const vr_camera *cam,
                                const vr_render_params *params, const vr_projection *proj, float *rgba_dev, void *stream);
vr_status vr_raycast_pool_projection(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                                     const int64_t grid[3], const vr_camera *cam, const vr_render_params *params,
                                     const vr_projection *proj, float *rgba_dev, void *stream);
vr_status vr_raycast_projection_partial(const uint8_t *volume_dev, const int64_t dims[3], const vr_camera *cam,
                                        const vr_render_params *params, const vr_projection *proj, float *partial_dev,
                                        void *stream);
vr_status vr_raycast_pool_projection_partial(const uint8_t *pool_dev, const vr_pool_entry *table_dev,
                                             const int64_t brick_dims[3], const int64_t grid[3], const vr_camera *cam,
                                             const vr_render_params *params, const vr_projection *proj, float *partial_dev,
                                             void *stream);
/* combine: front = combine(front, back); finish: the finish; slabs: the num_slabs partials of num_pixels pixels, stacked
 * back to back, combined in ascending index and finished -- no camera, axis or first_pixel, because order does not
 * matter.  VR_ERR_INVALID for a null pointer, num_pixels < 1, num_slabs < 1, an op outside 0..2 or a proj that
 * vr_raycast_projection would refuse. */
vr_status vr_composite_combine_proj(float *front_dev, const float *back_dev, int64_t num_pixels, int32_t op, void *stream);
vr_status vr_composite_finish_proj(const float *partial_dev, const vr_projection *proj, float *rgba_dev, int64_t num_pixels,
                                   void *stream);
vr_status vr_composite_slabs_proj(const float *partials_dev, int32_t num_slabs, int64_t num_pixels, const vr_projection *proj,
                                  float *rgba_dev, void *stream);

/* ---- slice views (new): oblique planes and thick slabs of a dense volume, exact across GPUs ------------------------------
 * A slice is a parallelepiped of samples, width x height pixels by `layers` layers, in texture space; it produces a
 * projection partial and finishes through the projection's finish.  layers == 1 is a thin slice, more layers are a thick
 * slab reduced by proj->op.  No camera, no render params and no render mode are involved.
 * Sample (px, py, l) sits at
 *   pos_k = ((origin_k + (float)px * du_k) + (float)py * dv_k) + (float)l * dw_k        (k = x, y, z)
 * with every product and sum rounded to float32, in that order.  A position is never accumulated by repeated addition:
 * a sample depends neither on its neighbours nor on the launch shape.
 * A sample is TAKEN iff vr_raycast's inside(pos) holds (strictly inside the unit cube) and pos lies in
 * [box_min, box_max) on every axis.  Its value:
 *   VR_SLICE_LINEAR   vr_raycast's trilinear fetch at pos, bit for bit;
 *   VR_SLICE_NEAREST  (float)voxel * (1.0f / 255.0f) of voxel clamp((int)floorf(pos_k * (float)G_k), 0, G_k - 1) of the
 *                     global volume (G = global_dims, or dims), located in the local volume as the fetch locates its taps
 *                     (minus vol_origin, clamped to the local extents).
 * Per pixel, n is the number of taken samples and v their maximum (a running maximum from 0), their minimum (from +inf) or
 * their float32 sum in ascending l.  The partial is (v, (float)n, 0, 0), or (0, 0, 0, 0) where n == 0; the frame is the
 * projection FINISH of that partial (the same function, not a copy), so vr_composite_finish_proj(partial) equals the
 * frame bit for bit, and the partials of slabs combine through vr_composite_combine_proj / _slabs_proj /
 * vr_compositor_composite_proj unchanged: MAX and MIN at any layer count, and every op at layers == 1 (one sample per
 * pixel has one owner), equal the single-GPU partial and frame bit for bit; MEAN of a thick slab has an exact n and a v
 * within two summation orders.  A rank's slab holds ONE halo layer, for both filters (NEAREST reads the voxel a position
 * falls into, which lies in the owner's slab; the halo only matters to LINEAR's second tap, but the layout is one).
 * There is no skip grid: at most `layers` fetches per pixel.  Row 0 of the frame is the row of `origin`. */
enum { VR_SLICE_NEAREST = 0, VR_SLICE_LINEAR = 1 };

typedef struct vr_slice_plane {
    int32_t width, height;      /* > 0 */
    int32_t layers;             /* 1 .. 2^24 (n stays exact in a float) */
    int32_t filter;             /* VR_SLICE_* */
    float origin[3];            /* texture-space centre of pixel (0,0), layer 0; row 0 = top */
    float du[3], dv[3], dw[3];  /* texture-space step per column, per row, per layer */
    float box_min[3], box_max[3];          /* ownership box, {0,0,0}-{1,1,1} on one GPU */
    int64_t global_dims[3], vol_origin[3]; /* as vr_render_params: 0 / 0 on one GPU */
} vr_slice_plane;               /* 136 bytes */

/* VR_ERR_INVALID (nothing launched) for a null pointer; width, height < 1; layers outside 1 .. 2^24; a filter that is
 * neither value; a non-finite origin, du, dv, dw or box; dims as vr_raycast refuses them; a proj that
 * vr_raycast_projection would refuse.  Then VR_ERR_NO_DEVICE: there is no CPU fallback.  volume_dev may start at any
 * byte; rgba_dev / partial_dev at any 4-byte-aligned address (a frame may be a view at any float of an allocation: no
 * 16-byte alignment is asked for, and nothing outside the width * height * 4 floats is written).  The _partial call writes
 * the partial instead of the frame: of proj it uses the op. */
vr_status vr_reslice(const uint8_t *volume_dev, const int64_t dims[3], const vr_slice_plane *plane, const vr_projection *proj,
                     float *rgba_dev, void *stream);
vr_status vr_reslice_partial(const uint8_t *volume_dev, const int64_t dims[3], const vr_slice_plane *plane,
                             const vr_projection *proj, float *partial_dev, void *stream);
/* Sort-last compositing of VR_RENDER_PARTIAL images: front = front OVER back, per pixel
 * (c1 + t1*c2, t1*t2); and the final colour transfer of raycaster.frag:82-85. */
vr_status vr_composite_over(float *front_dev, const float *back_dev, int64_t num_pixels, void *stream);
vr_status vr_composite_finish(const float *partial_dev, float *rgba_dev, int64_t num_pixels, void *stream);
/* Direct-send sort-last compositing of one image tile: partials_dev holds num_slabs partial images
 * of this tile back to back (num_pixels*4 floats each, slab s = the s-th slab along `axis` of the
 * volume).  Every pixel combines them front to back in ITS view order (ascending slab index where
 * the pixel's ray direction along `axis` is >= 0, descending otherwise -- "over" is associative but
 * not commutative) and applies the colour transfer.  first_pixel = row-major index of the tile's
 * first pixel in the width*height frame described by params. */
vr_status vr_composite_slabs(const float *partials_dev, int32_t num_slabs, int64_t num_pixels, int64_t first_pixel,
                             int32_t axis, const vr_camera *cam, const vr_render_params *params, float *rgba_dev,
                             void *stream);

/* ---- sort-last compositing across the GPUs of a node (new: the reference is single-GPU) ----------------
 * One process per GPU.  Rank r ray-marches slab r of the volume along `axis` into a VR_RENDER_PARTIAL image
 * (width * height * 4 floats); vr_compositor_composite moves tile t (a block of rows) of every rank's image to rank t
 * in ONE grouped RCCL call (ncclSend / ncclRecv over xGMI), combines the `world` partials of its tile per pixel in that
 * pixel's view order (vr_composite_slabs) and gathers the finished RGBA tiles on rank 0 (rgba_dev: width * height * 4
 * floats there, ignored elsewhere).  All of it is queued on `stream`.  The communicator is either the library's own,
 * created from an ncclUniqueId the ranks share (vr_rccl_unique_id on one rank, passed on by whatever the host uses
 * to talk between its processes), or the caller's ncclComm_t.  RCCL is bound at run time: world == 1 needs none, and
 * VR_ERR_UNSUPPORTED comes back where it cannot be found.  The alpha > 0.99 early exit of raycaster.frag:76 cannot be
 * honoured across slabs (bounded difference, <= 0.017 per channel). */
typedef struct vr_compositor vr_compositor;
vr_status vr_rccl_unique_id(uint8_t id[128]);
vr_status vr_compositor_create(vr_compositor **out, const uint8_t id[128], int32_t rank, int32_t world,
                               int32_t width, int32_t height);
vr_status vr_compositor_create_from_comm(vr_compositor **out, void *nccl_comm, int32_t rank, int32_t world,
                                         int32_t width, int32_t height);
vr_status vr_compositor_composite(vr_compositor *c, const float *partial_dev, int32_t axis, const vr_camera *cam,
                                  const vr_render_params *params, float *rgba_dev, void *stream);
/* vr_compositor_composite for the colour partials of vr_raycast_tf_partial: the same handle, buffers and exchange (the
 * same transport calls in the same order), the tile combined by vr_composite_slabs_tf.  Only tf->background is read.
 * With every rank's early exit on, the frame differs from the single-GPU one by at most 0.01 per channel (plus
 * rounding): a rank stops only once the frame's transmittance is below 0.01. */
vr_status vr_compositor_composite_tf(vr_compositor *c, const float *partial_dev, int32_t axis, const vr_camera *cam,
                                     const vr_render_params *params, const vr_transfer_function *tf, float *rgba_dev,
                                     void *stream);
/* vr_compositor_composite for the projection partials of vr_raycast_projection_partial: the same handle, buffers and
 * exchange (the same transport calls in the same order), the tile combined by vr_composite_slabs_proj.  No camera, axis
 * or params: the combine has no order.  The MAX and MIN frames equal the single-GPU frame bit for bit. */
vr_status vr_compositor_composite_proj(vr_compositor *c, const float *partial_dev, const vr_projection *proj, float *rgba_dev,
                                       void *stream);
vr_status vr_compositor_destroy(vr_compositor *c);
/* The transport seam: vr_compositor_composite's exchange is four point-to-point calls, made through this table.  RCCL
 * is the built-in table (ctx = the ncclComm_t) that the two constructors above install.  With
 * vr_compositor_create_with_transport the caller brings its own: every member gets `ctx` back, count is in floats,
 * stream is the one passed to vr_compositor_composite, and 0 means success.  The semantics are NCCL's grouped
 * point-to-point model -- send / recv only between group_start and group_end, the k-th send from p to r matches the
 * k-th recv on r from p, and the copies are ordered on `stream` (on both sides) without a host synchronisation.  The
 * seam exists so that the whole exchange can be tested on one GPU (tests/loopback_transport.cpp); a host may also use
 * it for another transport.  The compositor never destroys a caller's transport or ctx.
 * VR_ERR_INVALID for a null table or member, world < 1, a rank out of range or height < world; then
 * VR_ERR_NO_DEVICE without a GPU. */
typedef struct vr_transport {
    int32_t (*group_start)(void *ctx);
    int32_t (*group_end)(void *ctx);
    int32_t (*send)(void *ctx, const float *buf, int64_t count, int32_t peer, void *stream);
    int32_t (*recv)(void *ctx, float *buf, int64_t count, int32_t peer, void *stream);
} vr_transport;
vr_status vr_compositor_create_with_transport(vr_compositor **out, const vr_transport *t, void *ctx, int32_t rank,
                                              int32_t world, int32_t width, int32_t height);

/* ---- streams, events, pinned host memory (what include/vrhip/TimestepStreamer.hpp overlaps the stages of a timestep
 * stream with: main.cpp:242-290 runs them one after another).  Streams and events travel as void*. */
vr_status vr_stream_create(void **stream);
vr_status vr_stream_destroy(void *stream);
vr_status vr_stream_synchronize(void *stream);
vr_status vr_stream_wait_event(void *stream, void *event);
vr_status vr_event_create(void **event);
vr_status vr_event_destroy(void *event);
vr_status vr_event_record(void *event, void *stream);
vr_status vr_event_synchronize(void *event);
vr_status vr_event_elapsed_ms(void *start_event, void *end_event, float *ms);
vr_status vr_malloc_host(void **host, int64_t bytes);
vr_status vr_free_host(void *host);
vr_status vr_upload_async(void *dst_dev, const void *src_host, int64_t bytes, void *stream);
vr_status vr_download_async(void *dst_host, const void *src_dev, int64_t bytes, void *stream);

/* ---- instrumentation (the reference's DebugTimer phases, R.cpp:47-113) ----------
 * Milliseconds of the last build / decode measured with hipEvents on the call's stream:
 * phases[0..4] = BUILD(pyramid), COMPRESS, PRUNE, CONVERT, DECODE. */
vr_status vr_brickset_last_timings(vr_brickset *bs, float phases_ms[5]);

/* ---- concurrency inside one build (new; the reference's build(useThreads) is its nearest relative, R.cpp:17) ----
 * The level loop (compressGradientDescent) of a VolumeKdtree set is a chain of wide kernels and of one-wave-per-brick
 * control steps; run over `level_loop_streams` ranges of the bricks side by side (internal streams, forked from and
 * joined to the call's stream by events) the control steps of one range hide behind the wide kernels of another.
 * 1 = off, 2 = default, up to 4.  One build alone on the device: 2 is 5 % and 4 is 8 % faster than 1; with several
 * bricksets in flight on streams of their own, 1 is the right choice (the sets already fill each other's gaps).
 * Results do not depend on it.  MidRangeTree sets always run their two streams' level loops side by side. */
vr_status vr_brickset_set_concurrency(vr_brickset *bs, int32_t level_loop_streams);

/* ---- the contiguous stream (R.cpp:631-718, tree.swap(preorderTree)) ----------------------------------------------
 * A build of a brick of 4096 leaves or more keeps every 4096-leaf block's token string in a slot of its own (what the
 * decoders read, in place) and, as its last step, writes the reference's contiguous byte stream beside it: the bytes
 * vr_brickset_get_tree / save / get_packed4 hand out.  on_build = 0 leaves that copy to the first call that asks for
 * bytes (a pipeline that only ever decodes on the device saves ~4 % of a build); 1 (default) is the reference's build().
 * The contiguous streams of all bricks lie back to back in one buffer sized from their real lengths (about 0.6 byte
 * per voxel for the bench volume), regrown on demand. */
vr_status vr_brickset_set_compaction(vr_brickset *bs, int32_t on_build);

/* ---- debugging switches (new) ----------------------------------------------------------------------------------
 * Which kernel serves a call is decided by the set's geometry and by a few switches kept IN THE HANDLE: they are
 * initialised from the environment (VRHIP_DECODE_WALK, VRHIP_DECODE_FINE_V1, VRHIP_DECODE_QUAD, VRHIP_NO_SKIP_BLOCKS,
 * VRHIP_NO_UNIFORM_BLOCKS, VRHIP_NO_UNIFORM_DECODE, VRHIP_EST_EXACT_BOUNDS, VRHIP_EST_OLD_SCHEDULE, VRHIP_PYRAMID_BOXES)
 * once, when the set is created, and changed afterwards only through this call -- never by the environment at launch
 * time.  Names: "decode_walk", "decode_fine_v1", "decode_quad", "no_skip_blocks", "no_uniform_blocks",
 * "no_uniform_decode", "est_exact_bounds" (the distance estimator's quad rounds compute exact bounds per node instead
 * of sufficient ones per quad of nodes, and have no fallback budget), "est_old_schedule" (every round of the distance
 * estimator summarises a level to its end, under four candidate thresholds first, instead of a four-candidate round over
 * the level's first sixteenth, a two-candidate one up to a quarter and a one-candidate round over the bulk), "pyramid_boxes" (the pyramid's bottom twelve levels
 * by one 16^3 box per workgroup also where eight boxes per workgroup apply), "index_per_block" (the decode index of a
 * build by one wave per 4096-leaf block, not 32 blocks per workgroup); any other name is VR_ERR_INVALID.
 * Results never depend on a switch; the tests use them to check the kernels against each other.
 * vr_debug_set: process-wide switches that belong to no set: "skip_grid_v1"; "reslice_tile_w" = 8, 16 or 64, the width of
 * the 64-pixel tile a wave of vr_reslice covers (16 is the default, chosen by measurement: DESIGN.md 3.5g); "hist_plain" = 1
 * runs the histogram kernels without their data-aware paths (the same counts; DESIGN.md 3.5i prices them with it);
 * "mesh_count_only" = 1 makes vr_isomesh_count stop after its per-point pass -- it reports zero counts and leaves the
 * workspace unscanned -- so that profiles/tools/mesh_bench.py can price the scans. */
vr_status vr_brickset_set_switch(vr_brickset *bs, const char *name, int32_t value);
vr_status vr_debug_set(const char *name, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* VRHIP_H */
