// ptupsample.h — the arithmetic of ptss_upsample, written once for the gfx950 kernel (ptss_upsample.hip) and for
// the host probe (host_capi.cpp ptss_probe_upsample; tests/test_upsample_cpu.py): tap geometry, per-tap weight, accumulation order.
// Everything is float32 built from ptmath.h operations in the order written here, compiled without contraction on both sides, so
// the two builds agree bit for bit. The normal and depth terms of the weight, the depth slope and the byte conversion are
// ptdenoise.h's (tapExponent, slope, toByte), called, not restated.
//
// A joint-bilateral upsample of a W x H image to f W x f H, f = 1..4, guided by the features of both sizes. For hi pixel P = (X, Y)
// with feature F the centre in lo-pixel units is u = (X + 0.5) / f - 0.5, per axis and in integers (axisOf):
//     r = X mod f,  k = (2 r + 1 + f) mod 2 f,  x0 = X div f - (2 r + 1 < f),  fx = (float)k / (float)(2 f)      one IEEE division
// k is never f (2 r + 1 is odd), so the nearest lo pixel is unique; it is (X div f, Y div f) and always lies inside the frame.
// The four taps q = (x0 + i, y0 + j), i, j in {0, 1}, j outside and i inside; those outside the frame are skipped:
//     b_q = (i ? fx : 1 - fx) (j ? fy : 1 - fy)                                     the bilinear weight
//     w_q = b_q exp(-(e_normal + e_depth))   if materialIdx_q == materialIdx_P, else 0                      (the hard stop)
//     e_normal = max(0, 1 - n_P . n_q) / sigmaNormal
//     e_depth  = |z_P - z_q| / max(sigmaDepth (g_x a_x + g_y a_y) + 1e-3 z_P, 1e-30)
// (g_x, g_y): ptdn::slope of the HI-RES depth at P; (a_x, a_y): the tap's offset from P in hi pixels, k / 2 or (2 f - k) / 2, exact.
// Between two misses only b_q counts. A tap with !(w > 0) contributes nothing, not even to the clamp. With c_n the nearest tap's colour:
//     out = c_n + ( sum_q w_q (c_q - c_n) ) / ( sum_q w_q ),  clamped per channel to [min, max] of the counted c_q
// — the normalised sum written around c_n: a constant image stays constant exactly. No counted tap: out = c_n with weight 0, a
// surface the small frame did not see.
//
// upsamplePixel reads its four taps and four depth neighbours UNCONDITIONALLY, at coordinates clamped into the frame, before the
// first use of any of them, and decides afterwards which count: in the kernel every load is then in flight before the first wait
// (ptss_denoise.hip's waves wait 84 % of their cycles behind a load -> test -> load chain).
#pragma once
#include "ptdenoise.h"

namespace ptup {
using namespace ptv;

constexpr int kMaxFactor = PTSS_UPSAMPLE_MAX_FACTOR;   // 4 (ptss_types.h)
constexpr int kTileRows = 8;                            // hi-res rows per workgroup of the kernel: one grid row each
constexpr int kMaxHiRows = 65535 * kTileRows;           // the launch grid's second dimension ends at 65,535

struct Axis {   // one axis of the tap geometry of a hi pixel
    int x0;     // the lower tap, -1 .. size - 1
    int k;      // the centre's distance from it in units of 1 / (2 f) lo pixels = half hi pixels: 0 .. 2 f - 1, never f
    float f1;   // k / (2 f): the weight of tap x0 + 1
};

PTM_HD Axis axisOf(int X, int f) {
    const int r = X % f;
    Axis a;
    a.k = (2 * r + 1 + f) % (2 * f);
    a.x0 = X / f - (2 * r + 1 < f ? 1 : 0);
    a.f1 = ptm::div((float)a.k, (float)(2 * f));
    return a;
}

// the argument check ptss_upsample and ptss_probe_upsample share; nullptr when the parameters are acceptable
inline const char* paramsError(const ptss_upsample_params* p) {
    if (!p) return "params is null";
    if (p->structSize != (unsigned int)sizeof(ptss_upsample_params))
        return "params->structSize is not this library's sizeof(ptss_upsample_params): start from ptss_default_upsample_params";
    if (p->factor < 1 || p->factor > kMaxFactor) return "factor must be in [1, 4]";
    if (!(p->sigmaNormal > 0.0f && p->sigmaNormal < ptm::inf())) return "sigmaNormal must be finite and positive";
    if (!(p->sigmaDepth > 0.0f && p->sigmaDepth < ptm::inf())) return "sigmaDepth must be finite and positive";
    return nullptr;
}

// the constants of a call as ptdn::tapExponent takes them (its colour term is fed two equal colours and adds an exact 0)
inline ptdn::Level levelOf(const ptss_upsample_params& p) {
    ptdn::Level lv;
    lv.step = 1;
    lv.radius = 1;
    lv.invColor = 0.0f;
    lv.invNormal = 1.0f / p.sigmaNormal;
    lv.sigmaDepth = p.sigmaDepth;
    return lv;
}

struct Result {
    vec3 colour;    // on the 0..255 scale, before the byte conversion
    float weight;   // sum_q w_q; 0: no tap counted
};

PTM_HD vec3 colourOf(uint32_t rgba) { return v3((float)(rgba & 255u), (float)((rgba >> 8) & 255u), (float)((rgba >> 16) & 255u)); }
PTM_HD uint32_t packBytes(vec3 c) {   // uchar4 {x, y, z, w = 255}
    return (uint32_t)ptdn::toByte(c.x) | ((uint32_t)ptdn::toByte(c.y) << 8) | ((uint32_t)ptdn::toByte(c.z) << 16) | (255u << 24);
}

// Hi pixel (X, Y) of a width x height LO frame upsampled by f; fp: its hi-res feature. colourAt(q) -> uint32 (the lo image's RGBA
// word), featureAt(q) -> ptdn::Feature (lo), q = y * width + x; depthAt(X, Y) -> float, the hi-res depth of hi pixel (X, Y). Every
// accessor is called with coordinates inside its frame only.
template <class ColourAt, class FeatureAt, class DepthAt>
PTM_HD Result upsamplePixel(int X, int Y, int width, int height, int f, const ptdn::Level& lv, const ptdn::Feature& fp, ColourAt colourAt,
                            FeatureAt featureAt, DepthAt depthAt) {
    const Axis ax = axisOf(X, f), ay = axisOf(Y, f);
    // the loads: the nearest pixel, four taps and four depth neighbours, clamped into their frames
    const uint32_t nearest = colourAt((Y / f) * width + X / f);
    uint32_t word[4];
    ptdn::Feature fq[4];
    bool inside[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 4; ++t) {
        const int qx = ax.x0 + (t & 1), qy = ay.x0 + (t >> 1);
        inside[t] = qx >= 0 && qx < width && qy >= 0 && qy < height;
        const int cx = qx < 0 ? 0 : (qx >= width ? width - 1 : qx), cy = qy < 0 ? 0 : (qy >= height ? height - 1 : qy);
        const int q = cy * width + cx;
        word[t] = colourAt(q);
        fq[t] = featureAt(q);
    }
    const int hiW = width * f, hiH = height * f;
    const bool l = X > 0, r = X + 1 < hiW, d = Y > 0, u = Y + 1 < hiH;
    const float zl = depthAt(l ? X - 1 : X, Y), zr = depthAt(r ? X + 1 : X, Y), zd = depthAt(X, d ? Y - 1 : Y), zu = depthAt(X, u ? Y + 1 : Y);
#if defined(__HIP_DEVICE_COMPILE__)
    // An empty statement that reads one register of every load above: left alone, hipcc sinks a tap's loads behind the tests that
    // decide whether the tap counts (material, then colour, then geometry row, a wait before each). It changes no value.
    asm volatile("" ::"v"(word[0]), "v"(word[1]), "v"(word[2]), "v"(word[3]), "v"(fq[0].depth), "v"(fq[1].depth), "v"(fq[2].depth),
                 "v"(fq[3].depth), "v"(fq[0].materialIdx), "v"(fq[1].materialIdx), "v"(fq[2].materialIdx), "v"(fq[3].materialIdx), "v"(zl), "v"(zr),
                 "v"(zd), "v"(zu), "v"(nearest));
#endif

    // (selected, not branched on: a branch on F's material would put a wait between F's load and the loads above)
    const bool hit = fp.materialIdx >= 0;
    const float sx = ptdn::slope(fp.depth, l, zl, r, zr), sy = ptdn::slope(fp.depth, d, zd, u, zu);
    const float gx = hit ? sx : 0.0f, gy = hit ? sy : 0.0f;
    const vec3 cn = colourOf(nearest), zero = v3(0, 0, 0);
    vec3 sum = zero, lo = zero, hi = zero;
    float wsum = 0.0f;
    bool any = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 4; ++t) {
        const int i = t & 1, j = t >> 1;
        if (!inside[t] || fq[t].materialIdx != fp.materialIdx) continue;
        const float b = (i ? ax.f1 : 1.0f - ax.f1) * (j ? ay.f1 : 1.0f - ay.f1);
        const float offX = (float)(i ? 2 * f - ax.k : ax.k) * 0.5f, offY = (float)(j ? 2 * f - ay.k : ay.k) * 0.5f;
        const float e = ptdn::tapExponent(lv, zero, zero, fp, fq[t], gx, gy, offX, offY);
        const float w = b * ptm::exp(-e);
        if (!(w > 0.0f)) continue;   // an underflowed (or NaN) weight, or a bilinear weight of 0
        const vec3 cq = colourOf(word[t]);
        sum = madd(cq - cn, w, sum);
        wsum = wsum + w;
        lo = any ? v3(ptm::min(lo.x, cq.x), ptm::min(lo.y, cq.y), ptm::min(lo.z, cq.z)) : cq;
        hi = any ? v3(ptm::max(hi.x, cq.x), ptm::max(hi.y, cq.y), ptm::max(hi.z, cq.z)) : cq;
        any = true;
    }
    if (!any) return Result{cn, 0.0f};
    const vec3 out = cn + sum / wsum;
    return Result{v3(ptm::clamp(out.x, lo.x, hi.x), ptm::clamp(out.y, lo.y, hi.y), ptm::clamp(out.z, lo.z, hi.z)), wsum};
}

}  // namespace ptup
