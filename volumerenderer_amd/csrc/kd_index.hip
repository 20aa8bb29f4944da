// kd_index.hip -- the decode index of installed streams, rebuilt on the device (vr_brickset_set_trees).
//
// vr_brickset_set_tree parses a stream on the host, token by token, and uploads the index.  Here a stream comes with a
// block table (host_plan.h "block tables": where every 4096-leaf block's root token sits and which scalar its walk
// starts from), and one lane per block runs host_plan.h's index_block_walk -- the very function the CPU test program
// runs under the sanitizers -- over that block's tokens, then block_gap_walk over the tokens up to the next block.
// Together the lanes of a brick parse every token of its stream exactly once; any disagreement with the grammar or
// with the table's offsets raises the brick's flag.  Nothing read here is trusted: token reads are bounded by the
// stream's length, writes go to the block's own entries, and every loop consumes a token per iteration.
#include "brickset.h"

namespace vr {

struct IndexArgs {
    const uint8_t *tree;
    int64_t treeCap;
    const Ctrl *ctrls;
    const uint32_t *instOff;    // B * nBlk
    uint32_t *idxOff;
    uint8_t *idxVal, *fine, *val3, *top;
    int64_t nIdx;
    int D, K, nBlk;
    const int32_t *list;        // the call's bricks (grid rows); null: row = brick
    int32_t *flags;             // per row
};

// Index entries of the listed bricks back to "never installed": offsets dead, scalars and counts zero.  Not the heap
// of scalars: its upper levels were just copied from the table and the walkers write every other entry.
// onlyFlagged: the bricks whose flag is set (flags null: every listed brick), and then the heap and the control
// block's token count as well.
__global__ void __launch_bounds__(256)
k_index_reset(IndexArgs a, int onlyFlagged)
{
    const int row = blockIdx.y;
    const int brick = a.list ? a.list[row] : row;
    if (onlyFlagged && a.flags && a.flags[row] == 0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nIdx) return;
    const int64_t e = (int64_t)brick * a.nIdx + i;
    a.idxOff[e] = VR_IDX_DEAD;
    a.idxVal[e] = 0;
    if (a.fine) ((uint4 *)a.fine)[e] = make_uint4(0u, 0u, 0u, 0u);
    if (a.val3) ((uint2 *)a.val3)[e] = make_uint2(0u, 0u);
    if (onlyFlagged) {
        ((uint16_t *)a.top)[e] = 0;
        if (i == 0) const_cast<Ctrl *>(a.ctrls)[brick].numActive = 0ull;
    }
}

// One lane per block, 64 blocks per wave.  The value stack of a lane's walk (one byte per level Dc .. D) lives in LDS,
// [level][lane]; the map in LDS too.
__global__ void __launch_bounds__(64)
k_index_from_stream(IndexArgs a)
{
    __shared__ uint8_t stk[(VR_BLOCK_LEVELS + 1) * 64];
    __shared__ uint8_t dm[64];
    const int row = blockIdx.y, lane = threadIdx.x;
    const int brick = a.list ? a.list[row] : row;
    const Ctrl &c = a.ctrls[brick];
    if (lane <= a.D + VR_CHAIN_LEVELS) dm[lane] = c.distanceMap[lane];     // (D + 7 < VR_MAX_DEPTH = 40)
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;
    if (p >= a.nBlk) return;
    const unsigned long long na = c.numActive;
    int status = 0;
    if (na == 0ull || na >= (1ull << 32)) status = -1;
    else {
        const uint32_t *W = (const uint32_t *)(a.tree + (int64_t)brick * a.treeCap);
        const uint32_t *tab = a.instOff + (int64_t)brick * a.nBlk;
        const int Dc = block_depth(a.D);
        const bool fine = a.fine && a.K == 6 && a.D >= 6 && std_chain_distances(dm, a.D);    // (host_plan.h: other maps get no fine counts)
        BlockIndexOut o;
        o.off = a.idxOff + (int64_t)brick * a.nIdx;
        o.val = a.idxVal + (int64_t)brick * a.nIdx;
        o.fine = fine ? a.fine + (int64_t)brick * a.nIdx * 16 : nullptr;
        o.val3 = fine ? a.val3 + (int64_t)brick * a.nIdx * 8 : nullptr;
        o.top = a.top + (int64_t)brick * a.nIdx * 2;
        const uint32_t off = tab[p];
        // a live offset was checked on the host; a table changed since must still not send the walk anywhere
        if (off != VR_IDX_DEAD && off >= (uint32_t)na) status = -4;
        else {
            uint32_t end = 0;
            if (p == 0) status = block_gap_walk(W, (uint32_t)na, Dc, tab, -1, 0u);
            const int v0 = o.top[((int64_t)1 << Dc) + p];
            const int ws = index_block_walk(W, (uint32_t)na, dm, a.D, a.K, (uint32_t)p, off, v0, o, stk + lane, 64, &end);
            if (status == 0) status = ws;
            if (status == 0 && off != VR_IDX_DEAD) status = block_gap_walk(W, (uint32_t)na, Dc, tab, p, end);
        }
    }
    if (status != 0) atomicOr(a.flags + row, 1);
}

// cut < Ds: the scalar of every index entry's ancestor at the cut depth, from the heap
__global__ void __launch_bounds__(256)
k_cut_from_top(const uint8_t *__restrict__ top, int64_t nIdx, int Ds, int cut, const int32_t *__restrict__ list,
               const int32_t *__restrict__ cuts, int first, uint8_t *__restrict__ out)
{
    const int brick = list ? list[blockIdx.y] : first + (int)blockIdx.y;
    const int c = cuts ? cuts[brick] : cut;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nIdx || c < 0 || c >= Ds) return;
    out[(int64_t)brick * nIdx + i] = top[(int64_t)brick * nIdx * 2 + ((int64_t)1 << c) + (i >> (Ds - c))];
}

static IndexArgs index_args(BrickSet *bs, const int32_t *list, int32_t *flags)
{
    IndexArgs a;
    a.tree = bs->mid.tree; a.treeCap = bs->treeCap; a.ctrls = bs->mid.ctrl; a.instOff = bs->instOff;
    a.idxOff = bs->idxOff; a.idxVal = bs->idxVal; a.fine = bs->fineIdx; a.val3 = bs->idxVal3; a.top = bs->idxTop;
    a.nIdx = bs->nIdx; a.D = bs->D; a.K = bs->K; a.nBlk = 1 << block_depth(bs->D);
    a.list = list; a.flags = flags;
    return a;
}

int index_reset_launch(BrickSet *bs, const int32_t *list, int n, const int32_t *flags, bool onlyFlagged, hipStream_t st)
{
    if (n <= 0) return 0;
    const IndexArgs a = index_args(bs, list, const_cast<int32_t *>(flags));
    hipLaunchKernelGGL(k_index_reset, dim3((unsigned)((bs->nIdx + 255) / 256), (unsigned)n), dim3(256), 0, st, a, onlyFlagged ? 1 : 0);
    return launch_status("index_reset");
}

int index_from_stream_launch(BrickSet *bs, const int32_t *list, int n, int32_t *flags, hipStream_t st)
{
    if (n <= 0) return 0;
    const IndexArgs a = index_args(bs, list, flags);
    hipLaunchKernelGGL(k_index_from_stream, dim3((unsigned)((a.nBlk + 63) / 64), (unsigned)n), dim3(64), 0, st, a);
    return launch_status("index_from_stream");
}

int cut_from_top_launch(BrickSet *bs, const int32_t *list, const int32_t *cuts, int first, int n, int cut, uint8_t *out, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_cut_from_top, dim3((unsigned)((bs->nIdx + 255) / 256), (unsigned)n), dim3(256), 0, st,
                       bs->idxTop, bs->nIdx, bs->Ds, cut, list, cuts, first, out);
    return launch_status("cut_from_top");
}

} // namespace vr
