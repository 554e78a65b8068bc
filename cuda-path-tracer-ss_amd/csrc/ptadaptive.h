// ptadaptive.h — where the next round's samples go (ptss_plan_samples): the integer weight of a film pixel from its sums
// and its second moment, the targets that spread a budget of n rays over the running sum of the weights, and the search that turns a
// target into a pixel. PTM_HD over ptmath.h only: the host build of this header (libptss_host.so, ptss_probe_plan_samples) is the
// specification, the kernels of ptss_adaptive.hip evaluate the same operations in the same order, and the two agree byte for byte.
//
// Everything is unsigned 64-bit wrapping integer arithmetic or correctly rounded f32 (ptm::sqrt, ptm::div, round-to-nearest conversions),
// so inputs that do not belong together (moments of another film) still give one answer on both sides, and a weight of at most 2^19.
#ifndef PTSS_PTADAPTIVE_H
#define PTSS_PTADAPTIVE_H
#include "ptmath.h"

namespace ptad {

typedef unsigned long long u64;

constexpr uint32_t kUnsampledWeight = 1u << 19;   // a pixel below minSamples: it outranks every measured pixel (their cap is 2^19 - 1)
constexpr uint32_t kSampleLimit = 1u << 23;       // maxSamples <= 2^23: N < 2^23 keeps N * Q and S^2 below 195,075 * 2^46 < 2^64
constexpr float kWeightScale = 1024.f;            // weight = the standard error in 1/1024 of a display step
constexpr float kWeightCap = 524287.f;            // 2^19 - 1
constexpr int kScanTile = 2048;                   // pixels per workgroup of the device's scan (ptss_adaptive.hip): 256 lanes x 8
constexpr int kWorkspacePerTile = 3;              // 64-bit words of dev_cdf's tail per tile: its sum, active | unsampled << 32, capped

// what a pixel is to the plan
constexpr uint32_t kActive = 1u, kUnsampled = 2u, kCapped = 4u;

// the squared tone-mapped bytes of one sample: at most 3 * 255^2 = 195,075
PTM_HD uint32_t squares(uint32_t qr, uint32_t qg, uint32_t qb) { return qr * qr + qg * qg + qb * qb; }

// the weight of a pixel with sums (r, g, b) over N samples and second moment Q; *kind (may be null): kActive / kUnsampled / kCapped bits
PTM_HD uint32_t weight(uint32_t r, uint32_t g, uint32_t b, uint32_t N, u64 Q, uint32_t minSamples, uint32_t maxSamples, float threshold,
                       uint32_t* kind) {
    uint32_t w = 0u, k = 0u;
    if (N < minSamples) {
        w = kUnsampledWeight;
        k = kUnsampled;
    } else if (N >= maxSamples) {
        k = kCapped;
    } else {
        const u64 A = (u64)N * Q;
        const u64 B = (u64)r * (u64)r + (u64)g * (u64)g + (u64)b * (u64)b;
        const u64 D = A >= B ? A - B : 0ull;   // N^2 times the summed population variance of the three channels
        const float fn = (float)N;
        const float se = ptm::div(ptm::sqrt((float)D), fn * ptm::sqrt(fn));   // the standard error of the pixel's mean, 0..255 scale
        if (se > threshold) w = (uint32_t)ptm::min(se * kWeightScale, kWeightCap);   // (a NaN cannot arise: D and N are finite, N >= 1)
    }
    if (w > 0u) k |= kActive;
    if (kind) *kind = k;
    return w;
}

// the i-th of n targets over a total: floor((i * total + total / 2) / n) without an intermediate above 2^63 for total <= 2^50, n < 2^31
PTM_HD u64 target(u64 i, u64 n, u64 total) {
    const u64 q = total / n, r = total % n, h = total / 2ull;
    return i * q + (i * r + h) / n;
}

// the smallest p in [0, count) with cdf[p] > t; the caller guarantees cdf[count - 1] > t
PTM_HD uint32_t pixelOf(const u64* cdf, uint32_t count, u64 t) {
    uint32_t lo = 0u, hi = count - 1u;   // the answer lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (cdf[mid] > t) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

// every weight 1 (total = 0: nothing left to judge): the same rule over the pixel numbers themselves
PTM_HD uint32_t uniformPixel(u64 i, u64 n, u64 filmPixels) { return (uint32_t)((i * filmPixels + filmPixels / 2ull) / n); }

PTM_HD u64 scanTiles(u64 filmPixels) { return (filmPixels + (u64)kScanTile - 1ull) / (u64)kScanTile; }
PTM_HD u64 cdfEntries(u64 filmPixels) { return filmPixels + (u64)kWorkspacePerTile * scanTiles(filmPixels); }

// what ptss_plan_samples refuses about its parameters, or nullptr
inline const char* paramsError(const ptss_plan_params* p) {
    if (!p) return "params is null";
    if (p->structSize != sizeof(ptss_plan_params)) return "params->structSize is not sizeof(ptss_plan_params)";
    if (p->minSamples == 0u) return "minSamples must be at least 1";
    if (p->maxSamples == 0u || p->maxSamples > kSampleLimit) return "maxSamples must be in [1, 2^23]";
    if (p->maxSamples < p->minSamples) return "maxSamples must not be below minSamples";
    if (!(p->threshold >= 0.f) || !(p->threshold < ptm::inf())) return "threshold must be finite and not negative";
    return nullptr;
}

}  // namespace ptad
#endif
