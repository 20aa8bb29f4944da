// vrhip/BrickArchive.hpp -- compressed brick-set archives from C++: one file holds one brick set (one timestep) as its
// streams and their seek tables; opening or loading one installs every brick in one call and rebuilds the decode index
// on the GPU (vr_brickset_save_set / _open_set / _load_set / _load_set_memory; the layout and the rules are in vrhip.h,
// "compressed brick-set archives").  Plain C++14, host only.
#pragma once
#include "../vrhip.h"
#include <stdexcept>
#include <string>
#include <utility>

namespace vrhip {

// owns a vr_brickset handle
class BrickSetHandle {
public:
    BrickSetHandle() = default;
    explicit BrickSetHandle(vr_brickset *set) : set_(set) {}
    BrickSetHandle(const BrickSetHandle &) = delete;
    BrickSetHandle &operator=(const BrickSetHandle &) = delete;
    BrickSetHandle(BrickSetHandle &&o) noexcept : set_(o.set_) { o.set_ = nullptr; }
    BrickSetHandle &operator=(BrickSetHandle &&o) noexcept { std::swap(set_, o.set_); return *this; }
    ~BrickSetHandle() { if (set_) vr_brickset_destroy(set_); }
    vr_brickset *get() const { return set_; }
    explicit operator bool() const { return set_ != nullptr; }

private:
    vr_brickset *set_ = nullptr;
};

namespace archive {

inline void require(vr_status s, const char *what)
{
    if (s != VR_OK) throw std::runtime_error(std::string(what) + ": " + vr_status_string(s));
}

// a built set, or a set of installed streams, as one file
inline void save(vr_brickset *set, const std::string &path) { require(vr_brickset_save_set(set, path.c_str()), "vr_brickset_save_set"); }

// a new set from a file; synchronises `stream` once
inline BrickSetHandle open(const std::string &path, void *stream = nullptr)
{
    vr_brickset *set = nullptr;
    require(vr_brickset_open_set(&set, path.c_str(), stream), "vr_brickset_open_set");
    return BrickSetHandle(set);
}

// the next timestep into an existing set of the same geometry; synchronises `stream` once
inline void load(vr_brickset *set, const std::string &path, void *stream = nullptr)
{
    require(vr_brickset_load_set(set, path.c_str(), stream), "vr_brickset_load_set");
}

// ... from a file's bytes in host memory (16-byte aligned; pinned memory makes the copies asynchronous)
inline void load(vr_brickset *set, const void *blob_host, int64_t bytes, void *stream = nullptr)
{
    require(vr_brickset_load_set_memory(set, blob_host, bytes, stream), "vr_brickset_load_set_memory");
}

} // namespace archive
} // namespace vrhip
