// vrhip/CutError.hpp -- error-bounded level of detail from C++: ErrorTable, the host copy of what every cut of every
// brick of a set costs in accuracy (vr_brickset_error_table), and the selection of per-brick cuts under a bound
// (vr_lod_select_error).  The rule is in vrhip.h ("error-bounded level of detail").  Plain C++14, host only.
#pragma once
#include "../vrhip.h"
#include <stdexcept>
#include <string>
#include <vector>

namespace vrhip {

// rows cut_lo .. cut_hi of num_bricks entries each; owns the host table
class ErrorTable {
public:
    int32_t num_bricks = 0, cut_lo = 0, cut_hi = -1;
    int64_t voxels_per_brick = 0;
    std::vector<vr_brick_error> entries;

    int32_t num_cuts() const { return cut_hi - cut_lo + 1; }
    const vr_brick_error &at(int32_t cut, int32_t brick) const
    {
        if (cut < cut_lo || cut > cut_hi || brick < 0 || brick >= num_bricks) throw std::out_of_range("ErrorTable::at");
        return entries[(size_t)(cut - cut_lo) * (size_t)num_bricks + (size_t)brick];
    }
};

// The table of `set` (num_bricks bricks) for the cuts cut_lo .. cut_hi (cut_hi < 0: max_tree_depth) against
// reference_dev: the original voxels or any decode, in vr_brickset_build's layout.  scratch_dev: num_bricks * X*Y*Z bytes
// for the decodes, left with the decode at cut_hi.  Synchronises `stream`.
inline ErrorTable error_table(vr_brickset *set, const uint8_t *reference_dev, uint8_t *scratch_dev, int32_t num_bricks,
                              int32_t cut_lo = 0, int32_t cut_hi = -1, void *stream = nullptr)
{
    vr_tree_info ti;
    vr_status s = vr_brickset_info(set, 0, &ti);
    if (s != VR_OK) throw std::runtime_error(std::string("vr_brickset_info: ") + vr_status_string(s));
    ErrorTable t;
    t.num_bricks = num_bricks;
    t.cut_lo = cut_lo;
    t.cut_hi = cut_hi < 0 ? ti.max_tree_depth : cut_hi;
    t.voxels_per_brick = ti.X * ti.Y * ti.Z;
    if (num_bricks < 1 || t.cut_lo < 0 || t.cut_hi < t.cut_lo) throw std::invalid_argument("error_table: bricks or cuts");
    t.entries.resize((size_t)t.num_cuts() * (size_t)num_bricks);
    s = vr_brickset_error_table(set, reference_dev, scratch_dev, t.cut_lo, t.cut_hi, t.entries.data(), stream);
    if (s != VR_OK) throw std::runtime_error(std::string("vr_brickset_error_table: ") + vr_status_string(s));
    return t;
}

// Per-brick cuts under a bound: the smallest cut of the table, not above cuts_in[b] (geometry's choice, vr_lod_select;
// empty = the table's last cut), with max_abs <= max_abs_bound and, when mean_sq_bound >= 0, a mean squared error of at
// most mean_sq_bound.  The result goes to vr_brickset_decode_lod / _lod_pool as it is.
inline std::vector<int32_t> select_error_bounded(const ErrorTable &t, int32_t max_abs_bound = 0, double mean_sq_bound = -1.0,
                                                 const std::vector<int32_t> &cuts_in = std::vector<int32_t>())
{
    if (!cuts_in.empty() && (int64_t)cuts_in.size() != t.num_bricks) throw std::invalid_argument("select_error_bounded: cuts_in");
    std::vector<int32_t> cuts((size_t)(t.num_bricks > 0 ? t.num_bricks : 0));
    const vr_status s = vr_lod_select_error(t.entries.data(), t.num_bricks, t.cut_lo, t.cut_hi, t.voxels_per_brick,
                                            cuts_in.empty() ? nullptr : cuts_in.data(), max_abs_bound, mean_sq_bound,
                                            cuts.data());
    if (s != VR_OK) throw std::runtime_error(std::string("vr_lod_select_error: ") + vr_status_string(s));
    return cuts;
}

} // namespace vrhip
