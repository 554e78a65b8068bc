// ptmotion.h — the arithmetic of ptss_render_features_motion, written once for the gfx950 kernel (ptss_kernels.hip
// featureKernel<*, true>) and for the host probe (host_capi.cpp ptss_probe_motion; tests/test_motion_cpu.py). Everything is float32
// built from ptmath.h operations in the order written here, compiled without contraction on both sides, so the two builds agree
// bit for bit.
//
// Where was the surface point under a pixel's centre in the PREVIOUS pose? With d the pixel-centre direction, o the camera position
// and (kind, prim, dist, w1, w2) the closest hit of that ray (closestQuery / a ptss_ray_hit), prev the caller's previous records
// of triangles first .. first + count - 1 (19 words each, the 76-byte ptss_triangle):
//   miss:            prevPoint = 0, surface = -1
//   static hit:      prevPoint = fma(d, dist, o), surface = prim (a sphere) or 0x40000000 | prim (a triangle) — a sphere, a triangle
//                    outside the range, or a previous record that sceneUpdateKernel refuses (recordAccepted below: such a record
//                    never became geometry, the triangle stood where it stands). The expression is the one reprojectPixel
//                    (ptreproject.h) evaluates for the world point of a hit, so a static hit reprojects as ptss_reproject does.
//   moved triangle:  v0', v1', v2' of record prim - first; e1' = v1' - v0', e2' = v2' - v0' (one float subtraction per component,
//                    packTriangles'); prevPoint = fma(e2', w2, fma(e1', w1, v0')) — w1 goes with vertex1, w2 with vertex2
//                    (Primitives.h:58-73, the weights of the normal interpolation).
#pragma once
#include "ptmath.h"

namespace ptmo {
using namespace ptv;

constexpr int kTriangleWords = 19;             // sizeof(ptss_triangle) / 4
constexpr int kTriangleSurface = 0x40000000;   // ptss_pixel_motion::surface of triangle t: this | t
static_assert(sizeof(ptss_triangle) == kTriangleWords * 4, "ptss_triangle is 19 words");

// The acceptance test of ptss_update_triangles (sceneUpdateKernel): the nine vertex words of a record, every one finite and within
// |coordinate| <= 2^40 (false for NaN and infinities) — the mesh image's precondition.
PTM_HD bool recordAccepted(const float* r) {
    bool ok = true;
    for (int k = 0; k < 9; ++k) ok = ok && __builtin_fabsf(r[k]) <= 0x1p40f;
    return ok;
}

struct Motion {   // a ptss_pixel_motion
    vec3 prevPoint;
    int surface;
};

// prev is read only for a hit on a triangle inside the range: nine words of one record.
PTM_HD Motion pixelMotion(vec3 d, vec3 o, int kind, int prim, float dist, float w1, float w2, const float* prev, uint32_t first, uint32_t count) {
    const bool triangle = kind == PTSS_HIT_TRIANGLE;
    if (!triangle && kind != PTSS_HIT_SPHERE) return Motion{v3(0, 0, 0), -1};
    Motion m{madd(d, dist, o), triangle ? (kTriangleSurface | prim) : prim};
    if (triangle && (uint32_t)prim >= first && (uint32_t)prim - first < count) {
        const float* r = prev + (size_t)kTriangleWords * ((uint32_t)prim - first);
        float w[9];
        for (int k = 0; k < 9; ++k) w[k] = r[k];
        if (recordAccepted(w)) {
            const vec3 v0 = v3(w[0], w[1], w[2]);
            const vec3 e1 = v3(w[3], w[4], w[5]) - v0;
            const vec3 e2 = v3(w[6], w[7], w[8]) - v0;
            m.prevPoint = madd(e2, w2, madd(e1, w1, v0));
        }
    }
    return m;
}

}  // namespace ptmo
