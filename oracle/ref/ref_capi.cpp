// ref_capi.cpp -- TEST INFRASTRUCTURE ONLY: a C ABI over the reference codec
// itself, compiled in place from the reference's own sources into
// oracle/_ref/libvkref.so (see oracle/Makefile, target `ref`).  Nothing under
// volumerenderer_amd/ loads it; tests/test_ref_parity.py and
// tests/test_gpu_ref_parity.py compare the oracle and the HIP codec with it.
//
// The reference's two headers each define `byte`, MinMax and Point3i, so this
// file is compiled twice: once for class VolumeKdtree (prefix vkref_kd_) and
// once with -DVKREF_MIDRANGE for class MidRangeTree (prefix vkref_mid_).
//
// Two rules the wrapper keeps:
//  * build() swaps the caller's input vector empty, so every handle owns a
//    private copy of the voxels, and measureMaxError/measureMeanError (which
//    read through that emptied vector) are never called: errors are computed
//    from levelCut voxels by the caller.
//  * Only the serial build(false) is the pinned path.
// save() of an empty tree and open() of a missing file block on stdin or
// exit() in the reference; both are refused here before the call.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#ifdef VKREF_MIDRANGE
#include "MidRangeTree.h"
typedef MidRangeTree RefTree;
#define VKREF(name) vkref_mid_##name
#else
#include "VolumeKdtree_recover.h"
typedef VolumeKdtree RefTree;
#define VKREF(name) vkref_kd_##name
#endif

static_assert(sizeof(Point3i) == 3 * sizeof(int64_t), "the file layout writes Point3i verbatim");

namespace {

struct Handle {
    std::vector<byte> input;  // the reference's build() empties this; never read after
    RefTree tree;
    Handle() {}
    Handle(const uint8_t* vox, int64_t x, int64_t y, int64_t z)
        : input(vox, vox + x * y * z), tree(input, x, y, z) {}
};

Handle* H(void* h) { return static_cast<Handle*>(h); }

}  // namespace

extern "C" {

void* VKREF(create)(const uint8_t* vox, int64_t x, int64_t y, int64_t z) {
    if (!vox || x <= 0 || y <= 0 || z <= 0) return nullptr;
    return new (std::nothrow) Handle(vox, x, y, z);
}

void VKREF(destroy)(void* h) { delete H(h); }

void VKREF(set_error_tolerance)(void* h, int tol) { H(h)->tree.setErrorTolerance(tol); }
void VKREF(set_max_epochs)(void* h, int epochs) { H(h)->tree.setMaxEpochs(epochs); }

int VKREF(build)(void* h) {
    try {
        H(h)->tree.build(false);
    } catch (...) {
        return -1;
    }
    return 0;
}

int VKREF(max_tree_depth)(void* h) { return H(h)->tree.maxTreeDepth; }
int VKREF(orig_tree_depth)(void* h) { return H(h)->tree.origTreeDepth; }
int64_t VKREF(num_active_nodes)(void* h) { return H(h)->tree.numActiveNodes; }

void VKREF(dims)(void* h, int64_t* out) {
    out[0] = H(h)->tree.X;
    out[1] = H(h)->tree.Y;
    out[2] = H(h)->tree.Z;
}

int64_t VKREF(tree_bytes)(void* h) { return (int64_t)H(h)->tree.tree.bits.size(); }
const uint8_t* VKREF(tree_ptr)(void* h) { return H(h)->tree.tree.bits.data(); }
int64_t VKREF(distance_map_len)(void* h) { return (int64_t)H(h)->tree.distanceMap.size(); }
const uint8_t* VKREF(distance_map_ptr)(void* h) { return H(h)->tree.distanceMap.data(); }

#ifdef VKREF_MIDRANGE
int64_t VKREF(tree_range_bytes)(void* h) { return (int64_t)H(h)->tree.tree_range.bits.size(); }
const uint8_t* VKREF(tree_range_ptr)(void* h) { return H(h)->tree.tree_range.bits.data(); }
int64_t VKREF(distance_map_range_len)(void* h) { return (int64_t)H(h)->tree.distanceMap_range.size(); }
const uint8_t* VKREF(distance_map_range_ptr)(void* h) { return H(h)->tree.distanceMap_range.data(); }

// The 4-bit packing.  Returns its length; copies min(length, cap) bytes to out.
int64_t VKREF(convert_to_byte_array)(void* h, uint8_t* out, int64_t cap) {
    std::vector<byte> packed;
    H(h)->tree.convertToByteArray(packed);
    int64_t n = (int64_t)packed.size();
    if (out && cap > 0) std::memcpy(out, packed.data(), (size_t)(n < cap ? n : cap));
    return n;
}
#endif

int VKREF(save)(void* h, const char* path) {
    if (H(h)->tree.tree.bits.empty()) return -1;
    try {
        H(h)->tree.save(path);
    } catch (...) {
        return -2;
    }
    return 0;
}

void* VKREF(open)(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return nullptr;
    std::fclose(f);
    Handle* h = new (std::nothrow) Handle();
    if (!h) return nullptr;
    try {
        h->tree.open(path);
    } catch (...) {
        delete h;
        return nullptr;
    }
    return h;
}

// levelCut(cutDepth) into out[X*Y*Z], x fastest.  Only cutDepth == maxTreeDepth is pinned.
int VKREF(level_cut)(void* h, int cut_depth, uint8_t* out) {
    std::vector<byte> voxels;
    try {
        H(h)->tree.levelCut(cut_depth, voxels);
    } catch (...) {
        return -1;
    }
    if (!voxels.empty()) std::memcpy(out, voxels.data(), voxels.size());
    return 0;
}

}  // extern "C"
