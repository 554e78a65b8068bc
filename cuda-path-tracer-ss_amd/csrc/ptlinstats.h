// ptlinstats.h — adaptive sampling on the linear film (ptss_accumulate_paths_linear_stats / ptss_plan_samples_linear):
// the luminance moments of a sample in fixed point, and the integer weight of a pixel from the relative standard error of its mean
// luminance. PTM_HD over ptmath.h, ptlinear.h and ptmeter.h's luminance: the host build of this header (libptss_host.so,
// ptss_probe_accumulate_linear_stats / ptss_probe_plan_samples_linear / ptss_probe_linear_plan_weight) is the specification, the kernels of
// ptss_linear.hip evaluate the same operations in the same order, and the two agree byte for byte. Targets, search, uniform fallback and
// the workspace are ptadaptive.h's, unchanged: a weight is at most 2^19 here as there.
//
// A sample: q = ptlin::toFixed per channel (<= 2^40), y = ptmeter::luminance(q) <= 2^40, and y^2 <= 2^80 kept carry-save as
// lo = y^2 & (2^40 - 1), hi = y^2 >> 40 <= 2^40. A moment row sums y, lo, hi and the count: with fewer than 2^23 samples every word stays
// below 2^63; beyond that they wrap like any unsigned integer, on both sides alike.
//
// The weight works in unsigned 128-bit wrapping integers written out over two 64-bit words (no __int128: the device has none to lean on)
// and correctly rounded f32. For a consistent film (N < 2^23): Q = sqHi * 2^40 + sqLo <= N * 2^80 < 2^103, A = N * Q < 2^126,
// B = Sy^2 <= (N * 2^40)^2 < 2^126, and A >= B (Cauchy-Schwarz). Words that do not belong together wrap and still give one answer.
#ifndef PTSS_PTLINSTATS_H
#define PTSS_PTLINSTATS_H
#include "ptmath.h"
#include "ptlinear.h"
#include "ptmeter.h"
#include "ptadaptive.h"

namespace ptls {

using ptlin::u64;

constexpr u64 kLoMask = (1ull << 40) - 1ull;
constexpr float kWeightScale = 262144.f;   // 2^18: a relative error of 1 (the most a non-negative sample set can show) weighs 2^18
constexpr float kWeightCap = 524287.f;     // 2^19 - 1: below ptad::kUnsampledWeight

// an unsigned 128-bit integer
struct U128 {
    u64 lo, hi;
};

// the high 64 bits of a * b
PTM_HD u64 mulHi(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    const u64 a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
    const u64 p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const u64 mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);   // < 3 * 2^32
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
#endif
}

PTM_HD U128 mul64(u64 a, u64 b) { return U128{a * b, mulHi(a, b)}; }

// what one sample adds to a moment row
struct Sample {
    u64 y, lo, hi;
};

PTM_HD Sample sampleOf(u64 qr, u64 qg, u64 qb) {
    const u64 y = ptmeter::luminance(qr, qg, qb);
    const U128 sq = mul64(y, y);   // <= 2^80
    return Sample{y, sq.lo & kLoMask, (sq.lo >> 40) | (sq.hi << 24)};
}

// what the plan takes of its two parameter structs
struct Rule {
    uint32_t minSamples, maxSamples;
    float threshold;
    float floorFixed;   // floor * 2^scaleLog2 (exact), >= 1
};

// sqrt of a 128-bit integer as f32. D.hi = 0: the low word converted (round to nearest even) and rooted. Otherwise D is shifted right by
// an even s until it fits 64 bits, with bit 0 made sticky (so the one conversion rounds as the whole of D would), rooted, and scaled by
// 2^(s/2): exact, at most 2^64. (float)D itself could round to infinity.
PTM_HD float sqrt128(U128 D) {
    if (D.hi == 0ull) return ptm::sqrt((float)D.lo);
    int s = 64 - __builtin_clzll(D.hi);   // 1 .. 64
    s += s & 1;                           // 2 .. 64, even
    u64 m;
    bool lost;
    if (s == 64) {
        m = D.hi;
        lost = D.lo != 0ull;
    } else {
        m = (D.lo >> s) | (D.hi << (64 - s));
        lost = (D.lo & ((1ull << s) - 1ull)) != 0ull;
    }
    m |= lost ? 1ull : 0ull;
    return ptm::sqrt((float)m) * ptlin::pow2(s / 2);
}

// the standard error of the mean luminance of a moment row (Sy, sqLo, sqHi, N), N >= 1, in fixed-point units: what weight() divides by the
// mean, and what the linear denoiser (ptlindn.h) takes as a pixel's measured error
PTM_HD float standardError(u64 Sy, u64 sqLo, u64 sqHi, u64 N) {
    // Q = sqHi * 2^40 + sqLo
    U128 Q{sqHi << 40, sqHi >> 24};
    Q.lo += sqLo;
    Q.hi += Q.lo < sqLo ? 1ull : 0ull;
    // A = N * Q, B = Sy^2, both modulo 2^128
    U128 A = mul64(N, Q.lo);
    A.hi += N * Q.hi;
    const U128 B = mul64(Sy, Sy);
    const bool atLeast = A.hi > B.hi || (A.hi == B.hi && A.lo >= B.lo);
    U128 D{0ull, 0ull};   // N^2 times the population variance of the luminance
    if (atLeast) {
        D.lo = A.lo - B.lo;
        D.hi = A.hi - B.hi - (A.lo < B.lo ? 1ull : 0ull);
    }
    const float r = sqrt128(D);
    const float fn = (float)N;
    return ptm::div(r, fn * ptm::sqrt(fn));
}

// the weight of a pixel with moment row (Sy, sqLo, sqHi, N); *kind (may be null): ptad::kActive / kUnsampled / kCapped bits
PTM_HD uint32_t weight(u64 Sy, u64 sqLo, u64 sqHi, u64 N, const Rule& R, uint32_t* kind) {
    uint32_t w = 0u, k = 0u;
    if (N < (u64)R.minSamples) {
        w = ptad::kUnsampledWeight;
        k = ptad::kUnsampled;
    } else if (N >= (u64)R.maxSamples) {
        k = ptad::kCapped;
    } else {
        const float seY = standardError(Sy, sqLo, sqHi, N);
        const float fn = (float)N;
        const float meanY = ptm::div((float)Sy, fn);
        const float rel = ptm::div(seY, meanY + R.floorFixed);   // (the denominator is at least 1: no NaN, no division by zero)
        if (rel > R.threshold) w = (uint32_t)ptm::min(rel * kWeightScale, kWeightCap);
    }
    if (w > 0u) k |= ptad::kActive;
    if (kind) *kind = k;
    return w;
}

// what ptss_plan_samples_linear refuses about its parameters, or nullptr; `film` has passed ptlin::paramsError
inline const char* paramsError(const ptss_linear_plan_params* p, const ptss_linear_params* film) {
    if (!p) return "plan params is null";
    if (p->structSize != sizeof(ptss_linear_plan_params)) return "params->structSize is not sizeof(ptss_linear_plan_params)";
    if (p->minSamples == 0u) return "minSamples must be at least 1";
    if (p->maxSamples == 0u || p->maxSamples > ptad::kSampleLimit) return "maxSamples must be in [1, 2^23]";
    if (p->maxSamples < p->minSamples) return "maxSamples must not be below minSamples";
    if (!(p->threshold >= 0.f) || !(p->threshold < ptm::inf())) return "threshold must be finite and not negative";
    if (!(p->floor > 0.f) || !(p->floor < ptm::inf())) return "floor must be finite and positive";
    if (!(p->floor <= film->clampMax)) return "floor must not exceed clampMax";
    if (!(p->floor * ptlin::pow2(film->scaleLog2) >= 1.f)) return "floor * 2^scaleLog2 must be at least 1";
    if (p->reserved[0] != 0u || p->reserved[1] != 0u || p->reserved[2] != 0u) return "reserved must be 0";
    return nullptr;
}

inline Rule ruleOf(const ptss_linear_plan_params& p, const ptss_linear_params& film) {
    return Rule{p.minSamples, p.maxSamples, p.threshold, p.floor * ptlin::pow2(film.scaleLog2)};
}

}  // namespace ptls
#endif
