// frag_capi.cpp -- TEST INFRASTRUCTURE ONLY: a C ABI over the reference's two
// fragment shaders, compiled in place as C++14 into oracle/_ref/libvkfrag.so
// (see oracle/Makefile, target `ref`).  Nothing under volumerenderer_amd/ loads
// it; tests/test_ref_shader_parity.py and tests/test_gpu_ref_shader_parity.py
// compare the ray-march oracle and the HIP kernels with it.
//
// The Makefile generates three files into _ref/ (never committed):
//   raycaster_frag.inc, isosurface_frag.inc : the shader text without its
//       #version line, every floating literal given an `f` suffix (GLSL
//       literals are float32; as C++ they would be doubles, and `a > 0.99` or
//       `+= prev_alpha * 0.6` would round differently);
//   frag_literals.inc : one static_assert(sizeof(<literal> * 1.0f) ==
//       sizeof(float)) per floating literal token of those two files, so a
//       literal the rewrite missed stops the build.  -Werror=double-promotion
//       stops it as well wherever a double meets a float.
// ref/glsl.h is the stand-in for the GLSL types and built-ins; it says which
// choices are its own.  The shaders' globals become namespace-scope variables,
// so one call runs its fragments serially and calls must not overlap.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "glsl.h"

#define main shader_main
namespace glsl {
namespace raycaster {
#include "raycaster_frag.inc"
}
namespace isosurface {
#include "isosurface_frag.inc"
}
}  // namespace glsl
#undef main
#undef layout
#undef out
#undef in
#undef smooth
#undef uniform

#include "frag_literals.inc"

static_assert(sizeof(glsl::vec3) == 3 * sizeof(float) && sizeof(glsl::vec4) == 4 * sizeof(float), "packed vectors");

namespace {

// Binds the uniforms, then runs `shader` once per fragment with the `out` variable reset to 0.
int run(glsl::sampler3D& volume, glsl::vec3& camPos, glsl::vec3& stepSize, glsl::vec3& vUV, glsl::vec4& vFragColor,
        void (*shader)(), const uint8_t* vol, int64_t X, int64_t Y, int64_t Z, const float* cam_pos,
        const float* step_size, int64_t n, const float* vuv, float* frag) {
    if (!vol || X <= 0 || Y <= 0 || Z <= 0 || n < 0 || !cam_pos || !step_size || !vuv || !frag) return -1;
    volume = glsl::sampler3D{vol, X, Y, Z};
    camPos = glsl::vec3(cam_pos[0], cam_pos[1], cam_pos[2]);
    stepSize = glsl::vec3(step_size[0], step_size[1], step_size[2]);
    for (int64_t i = 0; i < n; ++i) {
        vUV = glsl::vec3(vuv[3 * i], vuv[3 * i + 1], vuv[3 * i + 2]);
        vFragColor = glsl::vec4(0.0f, 0.0f, 0.0f, 0.0f);
        shader();
        std::memcpy(frag + 4 * i, &vFragColor, 4 * sizeof(float));
    }
    return 0;
}

}  // namespace

extern "C" {

// n fragments of raycaster.frag: vuv[n][3] in, the raw vFragColor[n][4] out (not clamped: blue is 255).
// iso_value is unused (the shader has no such uniform); both entry points share one signature.
int vkfrag_raycaster(const uint8_t* vol, int64_t X, int64_t Y, int64_t Z, const float* cam_pos, const float* step_size,
                     float iso_value, int64_t n, const float* vuv, float* frag) {
    (void)iso_value;
    namespace S = glsl::raycaster;
    return run(S::volume, S::camPos, S::step_size, S::vUV, S::vFragColor, S::shader_main, vol, X, Y, Z, cam_pos,
               step_size, n, vuv, frag);
}

// n fragments of isosurface.frag; a zero gradient at a hit leaves NaN in the fragment, as the shader computes it.
int vkfrag_isosurface(const uint8_t* vol, int64_t X, int64_t Y, int64_t Z, const float* cam_pos, const float* step_size,
                      float iso_value, int64_t n, const float* vuv, float* frag) {
    namespace S = glsl::isosurface;
    S::isoValue = iso_value;
    return run(S::volume, S::camPos, S::step_size, S::vUV, S::vFragColor, S::shader_main, vol, X, Y, Z, cam_pos,
               step_size, n, vuv, frag);
}

// MAX_SAMPLES of the shader (0: raycaster, 1: isosurface)
int vkfrag_max_samples(int shader) { return shader == 0 ? glsl::raycaster::MAX_SAMPLES : glsl::isosurface::MAX_SAMPLES; }

// What a normalised fixed-point framebuffer keeps of a fragment: each channel clamped to [0, 1].  NaN stays NaN.
void vkfrag_framebuffer_clamp(const float* frag, float* rgba, int64_t nfloats) {
    for (int64_t i = 0; i < nfloats; ++i) rgba[i] = frag[i] < 0.0f ? 0.0f : (frag[i] > 1.0f ? 1.0f : frag[i]);
}

}  // extern "C"
