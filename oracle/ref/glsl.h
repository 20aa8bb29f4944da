// glsl.h -- TEST INFRASTRUCTURE ONLY: a stand-in for the part of GLSL 3.30 that
// the reference's raycaster.frag and isosurface.frag use, so that the two
// shaders compile as C++14 into oracle/_ref/libvkfrag.so (oracle/Makefile,
// target `ref`; C ABI in frag_capi.cpp).  Written for this recipe; it holds no
// reference text.
//
// What GLSL fixes, and this header follows:
//   * float is IEEE binary32; vec3/vec4 arithmetic is component-wise;
//   * sign(x) is 1, 0 or -1; max(x, y) is y where x < y, else x;
//   * dot(a, b) is a.x*b.x + a.y*b.y + a.z*b.z (the sum's order is the
//     stand-in's, left to right: GLSL does not fix it);
//   * an R8 texture reads as (v, 0, 0, 1).
// What GLSL leaves open, and is THE STAND-IN'S CHOICE (the reference does not
// pin these):
//   * texture(): the GL linear filter with clamp-to-edge, texel centres at
//     (i + 0.5) / N, R8 normalised as v * (1.0f / 255.0f), float32 weights,
//     interpolated along x, then y, then z as a + f * (b - a).  This is SURVEY C-8 and
//     tex3d() of raymarch_oracle.c; a GL driver may weight in fixed point.
//   * normalize(v) is v / sqrt(dot(v, v)): a zero vector gives non-finite
//     components (GLSL: undefined).
//   * pow() and sqrt() are the C library's powf / sqrtf.
//   * the `out` variable starts at 0 for every fragment (frag_capi.cpp resets
//     it; GLSL: undefined until written).
// The build adds -ffp-contract=off and no fast-math, and rewrites the shaders'
// floating literals to single precision (GLSL literals are float32; frag_capi.cpp
// holds the proof).
//
// vec4 overlays .x/.y/.z/.w, .r/.g/.b/.a and the .rgb the shaders assign
// through in one union, as vector libraries for C++ do; clang defines reads
// through the inactive member.
#ifndef VKFRAG_GLSL_H
#define VKFRAG_GLSL_H
#include <cmath>
#include <cstdint>

namespace glsl {

struct vec3 {
    union { float x, r; };
    union { float y, g; };
    union { float z, b; };
    vec3() = default;
    vec3(float s) : x(s), y(s), z(s) {}
    vec3(float a, float b_, float c) : x(a), y(b_), z(c) {}
};

struct vec4 {
    union {
        struct { float x, y, z, w; };
        struct { float r, g, b, a; };
        vec3 rgb;
    };
    vec4() = default;
    vec4(float a_, float b_, float c_, float d_) : x(a_), y(b_), z(c_), w(d_) {}
    vec4(vec3 v, float d_) : x(v.x), y(v.y), z(v.z), w(d_) {}
};

inline vec3 operator+(vec3 a, vec3 b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(vec3 a, vec3 b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(vec3 a, vec3 b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator+(vec3 a, float s) { return vec3(a.x + s, a.y + s, a.z + s); }
inline vec3 operator*(vec3 a, float s) { return vec3(a.x * s, a.y * s, a.z * s); }
inline vec3 operator*(float s, vec3 a) { return vec3(s * a.x, s * a.y, s * a.z); }
inline vec3 operator/(vec3 a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }
inline vec3 operator-(vec3 a) { return vec3(-a.x, -a.y, -a.z); }

inline float sign(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }
inline vec3 sign(vec3 v) { return vec3(sign(v.x), sign(v.y), sign(v.z)); }
inline float max(float x, float y) { return x < y ? y : x; }
inline float pow(float x, float y) { return ::powf(x, y); }
inline float dot(vec3 a, vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline vec3 normalize(vec3 v) { return v / ::sqrtf(dot(v, v)); }

struct sampler3D { const uint8_t* v; int64_t X, Y, Z; };

inline int64_t texel_clamp(int64_t i, int64_t n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

inline vec4 texture(const sampler3D& t, vec3 p) {
    float x = p.x * (float)t.X - 0.5f, y = p.y * (float)t.Y - 0.5f, z = p.z * (float)t.Z - 0.5f;
    float fx0 = ::floorf(x), fy0 = ::floorf(y), fz0 = ::floorf(z);
    float fx = x - fx0, fy = y - fy0, fz = z - fz0;
    int64_t xa = texel_clamp((int64_t)fx0, t.X), xb = texel_clamp((int64_t)fx0 + 1, t.X);
    int64_t ya = texel_clamp((int64_t)fy0, t.Y), yb = texel_clamp((int64_t)fy0 + 1, t.Y);
    int64_t za = texel_clamp((int64_t)fz0, t.Z), zb = texel_clamp((int64_t)fz0 + 1, t.Z);
    const float k = 1.0f / 255.0f;
    auto at = [&](int64_t i, int64_t j, int64_t l) { return (float)t.v[i + t.X * (j + t.Y * l)] * k; };
    float c000 = at(xa, ya, za), c100 = at(xb, ya, za), c010 = at(xa, yb, za), c110 = at(xb, yb, za);
    float c001 = at(xa, ya, zb), c101 = at(xb, ya, zb), c011 = at(xa, yb, zb), c111 = at(xb, yb, zb);
    float c00 = c000 + fx * (c100 - c000), c10 = c010 + fx * (c110 - c010);
    float c01 = c001 + fx * (c101 - c001), c11 = c011 + fx * (c111 - c011);
    float c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
    return vec4(c0 + fz * (c1 - c0), 0.0f, 0.0f, 1.0f);
}

}  // namespace glsl

// storage and layout qualifiers of the shaders' globals: plain namespace-scope variables here
#define layout(...)
#define out
#define in
#define smooth
#define uniform

#endif
