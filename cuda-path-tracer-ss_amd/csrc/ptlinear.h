// ptlinear.h — the linear film of a path query (ptss_accumulate_paths_linear / ptss_resolve_linear): a sample's linear
// radiance as 64-bit fixed point, and the resolve of a pixel's sums into its linear mean, its display pixel and its history entry.
// PTM_HD over ptmath.h and ptquant.h only: the host build of this header (libptss_host.so, ptss_probe_accumulate_linear /
// ptss_probe_resolve_linear) is the specification, the kernels of ptss_linear.hip evaluate the same operations in the same order, and the
// two agree byte for byte.
//
// A sample is clamped to [0, clampMax], scaled by 2^scaleLog2 (exact: a power of two, and clampMax * 2^scaleLog2 <= 2^40 keeps it finite),
// rounded to the nearest integer, ties to even, and added as an unsigned 64-bit integer: sums of integers do not depend on their order.
// A sample is at most 2^40, so a pixel's sums stay below 2^63 while it holds fewer than 2^23 samples (kSampleLimit); beyond that the sums
// wrap like any unsigned integer, on both sides alike. Everything except the two conversions and the one pow is integer work.
#ifndef PTSS_PTLINEAR_H
#define PTSS_PTLINEAR_H
#include "ptmath.h"
#include "ptquant.h"

namespace ptlin {

typedef unsigned long long u64;

constexpr int kMaxScaleLog2 = 32;
constexpr float kMaxScaled = 1099511627776.f;     // 2^40: the largest fixed-point sample
constexpr uint32_t kSampleLimit = 1u << 23;       // samples < 2^23 keep the sums below 2^63
constexpr float kIntegerFrom = 8388608.f;         // 2^23: every float at or above it is an integer

// 2^k for k in [-126, 127]
PTM_HD float pow2(int k) { return ptm::u2f((uint32_t)(127 + k) << 23); }

// what the kernels take of a ptss_linear_params
struct Scale {
    float clampMax;
    float up;         // 2^scaleLog2
    float down;       // 2^-scaleLog2
    float exposure;
};

// one channel of a sample: NaN -> 0 (*flag set), x < 0 (-inf, -0 included) -> 0, x > clampMax (+inf included) -> clampMax (*flag set)
PTM_HD u64 toFixed(float x, float clampMax, float up, uint32_t* flag) {
    const bool isNan = !(x == x);
    const bool above = x > clampMax;
    if (isNan || above) *flag = 1u;
    float v = above ? clampMax : x;
    v = v > 0.f ? v : 0.f;                    // NaN, the negatives and -0 leave here as +0
    float s = v * up;                         // exact, at most 2^40
    if (s < kIntegerFrom) s = (s + kIntegerFrom) - kIntegerFrom;   // the nearest integer, ties to even: the sum lies in [2^23, 2^24), where floats are the integers
    return (u64)s;                            // an integer already: the conversion is exact
}

// the three channels of one sample -> q[0..2]; returns 1 when a channel was NaN or above clampMax (negative channels do not count)
PTM_HD uint32_t sampleToFixed(float r, float g, float b, const Scale& sc, u64* q) {
    uint32_t flag = 0u;
    q[0] = toFixed(r, sc.clampMax, sc.up, &flag);
    q[1] = toFixed(g, sc.clampMax, sc.up, &flag);
    q[2] = toFixed(b, sc.clampMax, sc.up, &flag);
    return flag;
}

// the mean of a channel: (sum + N / 2) / N in unsigned 64-bit integers (exact), converted to float (round to nearest even) and
// multiplied by 2^-scaleLog2 (a multiply, on both sides; exact: the product of an integer-valued float >= 1 and 2^-32 at the least is normal)
PTM_HD float meanOf(u64 sum, u64 N, float down) {
    const u64 m = (sum + N / 2ull) / N;
    return (float)m * down;
}

// channel c of an entry shown from its mean: linear[c] = the mean itself, byte c of *word = the tone map of the exposed mean, hist[c] = its
// display value 0..255 (ptsplat.h resolves with the same expressions)
PTM_HD void showMean(float mean, int c, const Scale& sc, const float* T, float* linear, uint32_t* word, float* hist) {
    const float e = mean * sc.exposure;
    linear[c] = mean;
    *word |= ptq::quantize_fast(e, T) << (8 * c);
    hist[c] = 255.f * ptm::pow(ptm::clamp(e, 0.f, 1.f), ptm::kGamma);
}

// one film entry resolved. linear: the unexposed means and (float)N; px: the display pixel, the tone map of the exposed mean (uchar4 as
// one word, w = 255); hist: the display value 0..255 of the exposed mean and (float)N
PTM_HD void resolve(u64 r, u64 g, u64 b, uint32_t samples, const Scale& sc, const float* T, float* linear, uint32_t* px, float* hist) {
    if (samples == 0u) {
        linear[0] = linear[1] = linear[2] = linear[3] = 0.f;
        hist[0] = hist[1] = hist[2] = hist[3] = 0.f;
        *px = 255u << 24;
        return;
    }
    const u64 N = (u64)samples;
    const u64 sum[3] = {r, g, b};
    uint32_t word = 255u << 24;
    for (int c = 0; c < 3; ++c) showMean(meanOf(sum[c], N, sc.down), c, sc, T, linear, &word, hist);
    linear[3] = hist[3] = (float)samples;
    *px = word;
}

// what the linear calls refuse about their parameters, or nullptr
inline const char* paramsError(const ptss_linear_params* p) {
    if (!p) return "params is null";
    if (p->structSize != sizeof(ptss_linear_params)) return "params->structSize is not sizeof(ptss_linear_params)";
    if (p->scaleLog2 < 0 || p->scaleLog2 > kMaxScaleLog2) return "scaleLog2 must be in [0, 32]";
    if (!(p->clampMax > 0.f) || !(p->clampMax < ptm::inf())) return "clampMax must be finite and positive";
    if (!(p->clampMax * pow2(p->scaleLog2) <= kMaxScaled)) return "clampMax * 2^scaleLog2 must not exceed 2^40";
    if (!(p->exposure >= 0.f) || !(p->exposure < ptm::inf())) return "exposure must be finite and not negative";
    if (p->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

inline Scale scaleOf(const ptss_linear_params& p) { return Scale{p.clampMax, pow2(p.scaleLog2), pow2(-p.scaleLog2), p.exposure}; }

}  // namespace ptlin
#endif
