// ptdenoise.h — the arithmetic of ptss_denoise, written once for the gfx950 kernel (ptss_denoise.hip) and for
// the host probe (host_capi.cpp ptss_probe_denoise; tests/test_denoise_cpu.py): per-tap weight, accumulation order, the byte
// conversion. Everything is float32 built from ptmath.h operations in the order written here, compiled without contraction on
// both sides, so the two builds agree bit for bit.
//
// One pass (level i, tap spacing s = 2^i) of the edge-avoiding A-trous filter, for pixel p with colour c_p, feature f_p:
//     out = c_p + ( sum_q w_q (c_q - c_p) ) / ( sum_q w_q ),  clamped per channel to [min, max] of the c_q with w_q > 0
// over the 5x5 taps q = p + s (i, j), i, j in -2..2, inside the frame, rows j outward-in (-2 .. 2), i inside; w_p = h(0, 0).
// That is the normalised sum  sum w c / sum w  written around c_p: a constant image stays constant exactly, and the clamp keeps
// the result inside the convex hull of its taps whatever the rounding.
//     w_q = h(i) h(j) exp(-(e_colour + e_normal + e_depth))   if materialIdx_q == materialIdx_p, else 0  (the hard stop)
//     h = (3/8, 1/4, 1/16) for |i| = 0, 1, 2                                   the B3 spline
//     e_colour = |c_q - c_p|^2 / sigma_i^2,  sigma_i = sigmaColor 2^-i         (Dammertz et al. 2010: halves per level)
//     e_normal = max(0, 1 - n_p . n_q) / sigmaNormal                           falls with the angle between the normals
//     e_depth  = |z_p - z_q| / (sigmaDepth (g_x |s i| + g_y |s j|) + 1e-3 z_p) the depth step against what the local slope
//                (g_x, g_y) of p's depth — the smaller of the two one-pixel differences per axis — predicts for this offset:
//                the tolerance grows with the tap spacing and with the slope, so a floor seen at a grazing angle is filtered
//                along AND across its depth gradient, while a step between two surfaces of one material stops the tap
// Misses (materialIdx < 0) have no normal and an infinite depth: between two misses only e_colour counts.
#pragma once
#include "ptmath.h"
#include "ptss_types.h"

namespace ptdn {
using namespace ptv;

struct Level {   // the constants of one pass, evaluated on the host (levelOf) and handed to the kernel as they are
    int step;          // tap spacing 2^i
    int radius;        // 2; 0 for the pass of levels = 0, which only converts
    float invColor;    // 1 / sigma_i^2
    float invNormal;   // 1 / sigmaNormal
    float sigmaDepth;
};

inline Level levelOf(const ptss_denoise_params& p, int i) {
    Level lv;
    lv.step = 1 << i;
    lv.radius = p.levels > 0 ? 2 : 0;
    const float sigma = p.sigmaColor * (1.0f / (float)(1 << i));   // exact scaling
    lv.invColor = 1.0f / (sigma * sigma);
    lv.invNormal = 1.0f / p.sigmaNormal;
    lv.sigmaDepth = p.sigmaDepth;
    return lv;
}

struct Feature {   // what the filter reads of a ptss_pixel_feature
    vec3 normal;
    float depth;
    int materialIdx;
};

PTM_HD float spline(int k) { return k == 0 ? 0.375f : ((k == 1 || k == -1) ? 0.25f : 0.0625f); }

// the accumulator's entry as the colour the display shows, before the byte conversion (CudaTracer.cu:94-98)
PTM_HD vec3 displayValue(uint32_t r, uint32_t g, uint32_t b, float inverseTicks) {
    return v3((float)r * inverseTicks, (float)g * inverseTicks, (float)b * inverseTicks);
}
PTM_HD unsigned char toByte(float v) { return (unsigned char)(v + 0.5f); }

// |slope| of the depth along one axis at a pixel: the smaller one-pixel difference (an edge then takes the side that stays on
// the surface); 0 where neither neighbour gives a finite one
PTM_HD float slope(float z, bool hasA, float za, bool hasB, float zb) {
    const float a = hasA ? ptm::abs(z - za) : ptm::inf();
    const float b = hasB ? ptm::abs(zb - z) : ptm::inf();
    const float g = ptm::min(a, b);
    return g < ptm::inf() ? g : 0.0f;
}

// exponent of the tap weight; fp, fq of one material
PTM_HD float tapExponent(const Level& lv, vec3 cp, vec3 cq, const Feature& fp, const Feature& fq, float gx, float gy, float ax, float ay) {
    const vec3 dc = cq - cp;
    float e = dot(dc, dc) * lv.invColor;
    if (fp.materialIdx >= 0) {
        e = e + ptm::max(0.0f, 1.0f - dot(fp.normal, fq.normal)) * lv.invNormal;
        const float tol = ptm::max(ptm::fma(lv.sigmaDepth, ptm::fma(gx, ax, gy * ay), 1e-3f * fp.depth), 1e-30f);
        e = e + ptm::div(ptm::abs(fp.depth - fq.depth), tol);
    }
    return e;
}

// One pass for pixel (x, y). colourAt(index) -> vec3, featureAt(index) -> Feature, depthAt(index) -> float, index = y * width + x.
template <class ColourAt, class FeatureAt, class DepthAt>
PTM_HD vec3 filterPixel(int x, int y, int width, int height, const Level& lv, ColourAt colourAt, FeatureAt featureAt, DepthAt depthAt) {
    const int p = y * width + x;
    const vec3 cp = colourAt(p);
    if (lv.radius == 0) return cp;
    const Feature fp = featureAt(p);
    float gx = 0.0f, gy = 0.0f;
    if (fp.materialIdx >= 0) {
        const bool l = x > 0, r = x + 1 < width, d = y > 0, u = y + 1 < height;
        gx = slope(fp.depth, l, l ? depthAt(p - 1) : 0.0f, r, r ? depthAt(p + 1) : 0.0f);
        gy = slope(fp.depth, d, d ? depthAt(p - width) : 0.0f, u, u ? depthAt(p + width) : 0.0f);
    }
    vec3 sum = v3(0, 0, 0), lo = cp, hi = cp;
    float wsum = spline(0) * spline(0);
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * lv.step;
        if (qy < 0 || qy >= height) continue;
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * lv.step;
            if (qx < 0 || qx >= width || (i == 0 && j == 0)) continue;
            const int q = qy * width + qx;
            const Feature fq = featureAt(q);
            if (fq.materialIdx != fp.materialIdx) continue;
            const vec3 cq = colourAt(q);
            const float e = tapExponent(lv, cp, cq, fp, fq, gx, gy, (float)((i < 0 ? -i : i) * lv.step), (float)((j < 0 ? -j : j) * lv.step));
            const float w = (spline(i) * spline(j)) * ptm::exp(-e);
            if (!(w > 0.0f)) continue;   // an underflowed (or NaN) weight contributes nothing, not even to the clamp
            sum = madd(cq - cp, w, sum);
            wsum = wsum + w;
            lo = v3(ptm::min(lo.x, cq.x), ptm::min(lo.y, cq.y), ptm::min(lo.z, cq.z));
            hi = v3(ptm::max(hi.x, cq.x), ptm::max(hi.y, cq.y), ptm::max(hi.z, cq.z));
        }
    }
    const vec3 out = cp + sum / wsum;
    return v3(ptm::clamp(out.x, lo.x, hi.x), ptm::clamp(out.y, lo.y, hi.y), ptm::clamp(out.z, lo.z, hi.z));
}

}  // namespace ptdn
