// vrhip/Histogram.hpp -- what values a volume holds, from C++: Histogram, the host copy of the 256-bin tables of
// vr_histogram_bricks / vr_histogram_pool (per brick or cell, and in total), histogram2d, the joint table of value and
// gradient magnitude (vr_histogram2d), and window_from_histogram, a display window from a histogram's percentiles.
// The rule is in vrhip.h ("volume histograms").  Plain C++14, host only.
#pragma once
#include "../vrhip.h"
#include <stdexcept>
#include <string>
#include <vector>

namespace vrhip {

// the display window of a vr_projection: value / 255, 0 <= lo < hi <= 1
struct Window { float lo, hi; };

// parts[p * 256 + k]: the count of value k in part p (a brick, or a grid cell of a pool); total[k]: over all parts
class Histogram {
public:
    int64_t num_parts = 0;
    std::vector<uint32_t> parts;
    std::vector<uint64_t> total;

    uint32_t at(int64_t part, int value) const
    {
        if (part < 0 || part >= num_parts || value < 0 || value >= VR_HIST_BINS) throw std::out_of_range("Histogram::at");
        return parts[(size_t)part * VR_HIST_BINS + (size_t)value];
    }

    // num_bricks bricks of voxels_per_brick bytes back to back at data_dev (any byte offset).  Synchronises `stream`.
    static Histogram of_bricks(const uint8_t *data_dev, int32_t num_bricks, int64_t voxels_per_brick, void *stream = nullptr)
    {
        if (num_bricks < 1) throw std::invalid_argument("Histogram::of_bricks: num_bricks");
        Histogram h;
        h.resize(num_bricks);
        const vr_status s = vr_histogram_bricks(data_dev, num_bricks, voxels_per_brick, h.parts.data(), h.total.data(), stream);
        if (s != VR_OK) throw std::runtime_error(std::string("vr_histogram_bricks: ") + vr_status_string(s));
        return h;
    }

    // the virtual volume of a pool (what vr_raycast_pool reads), one part per grid cell, x fastest
    static Histogram of_pool(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                             const int64_t grid[3], void *stream = nullptr)
    {
        if (!grid || grid[0] < 1 || grid[1] < 1 || grid[2] < 1 || grid[0] * grid[1] >= (1ll << 31) / grid[2])
            throw std::invalid_argument("Histogram::of_pool: grid");
        Histogram h;
        h.resize(grid[0] * grid[1] * grid[2]);
        const vr_status s = vr_histogram_pool(pool_dev, table_dev, brick_dims, grid, h.parts.data(), h.total.data(), stream);
        if (s != VR_OK) throw std::runtime_error(std::string("vr_histogram_pool: ") + vr_status_string(s));
        return h;
    }

private:
    void resize(int64_t n)
    {
        num_parts = n;
        parts.assign((size_t)n * VR_HIST_BINS, 0u);
        total.assign(VR_HIST_BINS, 0ull);
    }
};

// The VR_HIST_GRAD_BINS x VR_HIST_BINS table of the voxels [own_lo, own_hi) (global coordinates; null: all that
// volume_dev holds) of a volume of global_dims voxels (null: dims) of which volume_dev holds [vol_origin, vol_origin +
// dims) (null: the origin).  Entry r * 256 + v.  Synchronises `stream`.
inline std::vector<uint64_t> histogram2d(const uint8_t *volume_dev, const int64_t dims[3], const int64_t *global_dims = nullptr,
                                         const int64_t *vol_origin = nullptr, const int64_t *own_lo = nullptr,
                                         const int64_t *own_hi = nullptr, void *stream = nullptr)
{
    if (!dims) throw std::invalid_argument("histogram2d: dims");
    int64_t g[3], o[3], lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        g[k] = global_dims ? global_dims[k] : 0;
        o[k] = vol_origin ? vol_origin[k] : 0;
        lo[k] = own_lo ? own_lo[k] : o[k];
        hi[k] = own_hi ? own_hi[k] : o[k] + dims[k];
    }
    std::vector<uint64_t> hist((size_t)VR_HIST_GRAD_BINS * VR_HIST_BINS, 0ull);
    const vr_status s = vr_histogram2d(volume_dev, dims, g, o, lo, hi, hist.data(), stream);
    if (s != VR_OK) throw std::runtime_error(std::string("vr_histogram2d: ") + vr_status_string(s));
    return hist;
}

// The window between two percentiles of a 256-bin histogram, counting the bins from first_bin on (1 leaves the
// background out): what vr_projection's window_lo / window_hi take.
inline Window window_from_histogram(const std::vector<uint64_t> &hist, int32_t first_bin = 0, double lo_fraction = 0.01,
                                    double hi_fraction = 0.99)
{
    if (hist.size() != (size_t)VR_HIST_BINS) throw std::invalid_argument("window_from_histogram: 256 counts");
    Window w{0.0f, 1.0f};
    const vr_status s = vr_window_from_histogram(hist.data(), first_bin, lo_fraction, hi_fraction, &w.lo, &w.hi);
    if (s != VR_OK) throw std::runtime_error(std::string("vr_window_from_histogram: ") + vr_status_string(s));
    return w;
}

} // namespace vrhip
