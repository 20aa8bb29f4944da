// vrhip/TransferFunction.hpp -- a transfer-function table for vr_raycast_tf / vr_raycast_pool_tf from control points,
// without Python: the rule of volumerenderer_amd.render.transfer_function_table.  Plain C++14, host only.
#pragma once
#include "../vrhip.h"
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

namespace vrhip {

struct TfPoint { double value, r, g, b, a; };      // value in [0, 255], colours in [0, 1]

// 256 x (r, g, b, a) float32, entry k for the scalar k / 255.  The points are sorted by value (non-decreasing).  Entry
// k is linear between the last point at or below k and the point after it, the first point's colour below the first
// value and the last point's from the last value on; computed in double and rounded to float.  Throws
// std::invalid_argument for an empty list, unsorted values, a value outside [0, 255] or a colour outside [0, 1].
inline std::vector<float> transfer_function_from_points(const std::vector<TfPoint> &pts)
{
    if (pts.empty()) throw std::invalid_argument("transfer function: no control points");
    for (size_t i = 0; i < pts.size(); ++i) {
        const TfPoint &p = pts[i];
        const double c[5] = {p.value, p.r, p.g, p.b, p.a};
        for (double q : c)
            if (!std::isfinite(q)) throw std::invalid_argument("transfer function: point " + std::to_string(i) + " is not finite");
        if (!(p.value >= 0.0 && p.value <= 255.0)) throw std::invalid_argument("transfer function: point " + std::to_string(i) + ": value outside [0, 255]");
        for (int k = 1; k < 5; ++k)
            if (!(c[k] >= 0.0 && c[k] <= 1.0)) throw std::invalid_argument("transfer function: point " + std::to_string(i) + ": r, g, b, a outside [0, 1]");
        if (i && p.value < pts[i - 1].value) throw std::invalid_argument("transfer function: points are not sorted by value");
    }
    std::vector<float> lut(256 * 4);
    const int n = (int)pts.size();
    int j = -1;                                     // the last point at or below k
    for (int k = 0; k < 256; ++k) {
        while (j + 1 < n && pts[j + 1].value <= k) ++j;
        const TfPoint &p0 = pts[j < 0 ? 0 : j];
        const double c0[4] = {p0.r, p0.g, p0.b, p0.a};
        if (j < 0 || j + 1 == n) {
            for (int c = 0; c < 4; ++c) lut[4 * k + c] = (float)c0[c];
            continue;
        }
        const TfPoint &p1 = pts[j + 1];
        const double c1[4] = {p1.r, p1.g, p1.b, p1.a};
        const double t = (k - p0.value) / (p1.value - p0.value);
        for (int c = 0; c < 4; ++c) lut[4 * k + c] = (float)(c0[c] + t * (c1[c] - c0[c]));
    }
    return lut;
}

// the lighting volumerenderer_amd.render.Shading() defaults to: ka 0.3, kd 0.7, ks 0.2, shininess 32, head light,
// grad_min 1/255
inline vr_shading default_shading()
{
    vr_shading s;
    s.ambient = 0.3f; s.diffuse = 0.7f; s.specular = 0.2f; s.shininess = 32.0f;
    s.light_dir[0] = s.light_dir[1] = s.light_dir[2] = 0.0f;
    s.grad_min = (float)(1.0 / 255.0);
    return s;
}

} // namespace vrhip
