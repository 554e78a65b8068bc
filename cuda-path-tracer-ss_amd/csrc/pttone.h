// pttone.h — tone curves for the two linear films (ptss_tone_build / ptss_resolve_toned): a curve (the clamp, Reinhard
// with a white point, a filmic rational), a transfer function (the 2.2 power, sRGB) and a bit depth (8 or 10), the table of thresholds
// that describes their quantised composition, and the resolve of a film entry through that table. PTM_HD over ptmath.h, ptquant.h,
// ptlinear.h (and ptsplat.h, ptmeter.h, ptglare.h for the means a resolve shows): the host build of this header (libptss_host.so,
// ptss_probe_tone_*) is the specification, the kernels of ptss_tone.hip evaluate the same operations in the same order, and the two agree
// byte for byte. It generalises ptquant.h, which does this once for the reference's tone map.
//
//   display value   v = transfer(curve(x)) in float32:
//       saturation    x > 2^40 -> 2^40, x < 0 -> +0 (NaN and -0 pass). 2^40 is the largest fixed-point sample (ptlin::kMaxScaled): a film's
//                     mean times any sane exposure stays below it. With it curve(+inf) is curve(2^40), the rational forms never see inf / inf
//                     for parameters that paramsError accepts (below), and no input that is not NaN yields NaN. The lower bound makes the
//                     display value of a negative input that of 0, which is the level the table gives it
//       CLAMP         c = clamp(x, 0, 1)
//       REINHARD      c = clamp(div(x * fma(x, rcpWhite2, 1), 1 + x), 0, 1), rcpWhite2 = div(1, white * white) once on the host
//       FILMIC        c = clamp(div(x * fma(a, x, b), fma(x, fma(c, x, d), e)), 0, 1)
//       GAMMA22       v = pow(c, kGamma)
//       SRGB          v = c <= 0.0031308f ? 12.92f * c : fma(1.055f, pow(c, 1 / 2.4f), -0.055f)
//   level           L(x) = (uint)clamp(K v + 0.5f, 0, K), NaN -> 0, K = 255 or 1023: ptq::quantize_literal's form
//   table           T[0] = -inf; T[k], k = 1 .. K: the float of smallest bit pattern in [+0, +inf] with L >= k, by 31 steps of bisection over
//                   the bit patterns (non-negative floats order like their patterns), NaN where L(+inf) < k; T[K + 1] = NaN; T[K + 2] =
//                   the number 0 where T[1..K] is non-decreasing with its NaNs at the tail, 1 where it is not ("unsorted": both builders
//                   write it, the host's also returns it); T[K + 3] = T[K + 4] = NaN. K + 5 = 2^bits + 4 floats: whole float4 rows
//   THE TABLE IS THE SPECIFICATION OF THE PIXEL: the level of x is the number of k in 1 .. K with x >= T[k]. NaN and negatives give 0 and a
//   NaN entry never counts.
//
// Why the table is sorted although float32 rounding can make L non-monotone by an ulp here and there. First, what keeps a table
// meaningful: T[k + 1] < T[k] would need L to fall by more than a whole level; L is the floor of K v + 0.5, and the rounding noise of
// K v + 0.5 is a few ulps of a number below 1024, some 1e-4 at most, against the 1 that a whole level needs, so where the exact curve
// does not fall (the clamp and Reinhard never do) every threshold is THE place where L passes k. Second, what makes the order hold for
// any L whatever, a filmic[] whose rational rises and falls again (a = 0, say) included: all bisections walk the same midpoints
// from the same first interval, and L(mid) >= k + 1 implies L(mid) >= k, so the walk for k goes left wherever the walk for k + 1 does;
// where the two part, the one for k has gone left of a midpoint and the one for k + 1 right of it: T[k] <= mid < T[k + 1]. The end
// tests agree in the same way (L(+0) >= k + 1 implies L(+0) >= k; L(+inf) < k implies L(+inf) < k + 1: NaNs only at the tail). The
// builders check the order all the same and write the flag, so that a caller does not have to take this on trust and a change to the
// walk that broke it could not pass silently. levelSearch below relies on the order; levelCount does not.
//
// Per channel (PTSS_TONE_LUMINANCE clear): x_c = e_c = mean_c * exposure, the table is built from the curve and the transfer.
// Luminance (set): Y = fma(e_b, 19/256.f, fma(e_g, 183/256.f, e_r * (54/256.f))) (ptlindn.h's luminance), s = Y > 0 ? div(curve(Y), Y) : 0,
// x_c = e_c * s, and the table is built from CLAMP and the transfer: the curve moves the luminance, the channels keep their ratios until
// the clamp. history[c] = 255.f * the display value of x_c under the stage the table encodes, at either bit depth.
#ifndef PTSS_PTTONE_H
#define PTSS_PTTONE_H
#include "ptmath.h"
#include "ptquant.h"
#include "ptlinear.h"
#include "ptsplat.h"
#include "ptmeter.h"
#include "ptglare.h"

namespace pttone {

using ptlin::u64;

constexpr float kSaturate = ptlin::kMaxScaled;   // 2^40
constexpr float kSrgbKnee = 0.0031308f, kSrgbSlope = 12.92f, kSrgbScale = 1.055f, kSrgbOffset = -0.055f, kSrgbPower = 1 / 2.4f;
constexpr float kLumR = 54 / 256.f, kLumG = 183 / 256.f, kLumB = 19 / 256.f;
constexpr int kBisectSteps = 31;   // [+0, +inf] holds 0x7f800001 patterns: hi - lo starts below 2^31

// top level of a bit depth, and the floats of its table (whole float4 rows: T[0 .. K], T[K + 1] NaN, T[K + 2] the flag, T[K + 3] and T[K + 4] NaN)
PTM_HD uint32_t topOf(int bits) { return bits == 10 ? 1023u : 255u; }
PTM_HD int tableFloats(int bits) { return (int)topOf(bits) + 5; }

// one stage: a curve and a transfer at a bit depth. What a table is built from, and what history shows
struct Stage {
    int curve, transfer;
    uint32_t K;
    float rcpWhite2;   // REINHARD
    float a, b, c, d, e;   // FILMIC
};

// what the kernels take of a ptss_tone_params: `shown` is the stage of the table and of history; `lum` the stage whose curve moves the
// luminance (luminance mode only; `shown` is then CLAMP with the same transfer)
struct Rule {
    Stage shown;
    Stage lum;
    uint32_t luminance;   // PTSS_TONE_LUMINANCE set
};

PTM_HD float saturate(float x) {
    x = x > kSaturate ? kSaturate : x;
    return x < 0.f ? 0.f : x;
}

PTM_HD float curveOf(const Stage& S, float x) {
    x = saturate(x);
    if (S.curve == PTSS_TONE_REINHARD) return ptm::clamp(ptm::div(x * ptm::fma(x, S.rcpWhite2, 1.f), 1.f + x), 0.f, 1.f);
    if (S.curve == PTSS_TONE_FILMIC) return ptm::clamp(ptm::div(x * ptm::fma(S.a, x, S.b), ptm::fma(x, ptm::fma(S.c, x, S.d), S.e)), 0.f, 1.f);
    return ptm::clamp(x, 0.f, 1.f);
}

PTM_HD float transferOf(const Stage& S, float c) {
    if (S.transfer == PTSS_TRANSFER_SRGB) return c <= kSrgbKnee ? kSrgbSlope * c : ptm::fma(kSrgbScale, ptm::pow(c, kSrgbPower), kSrgbOffset);
    return ptm::pow(c, ptm::kGamma);
}

// the literal display value and the literal level
PTM_HD float valueOf(const Stage& S, float x) { return transferOf(S, curveOf(S, x)); }

PTM_HD uint32_t levelLiteral(const Stage& S, float x) {
    const float top = (float)S.K;
    const float v = ptm::clamp(top * valueOf(S, x) + 0.5f, 0.f, top);
    return (v == v) ? (uint32_t)v : 0u;
}

// T[k], k in 1 .. K
PTM_HD float thresholdOf(const Stage& S, uint32_t k) {
    uint32_t lo = 0u, hi = 0x7f800000u;
    if (levelLiteral(S, ptm::u2f(lo)) >= k) return ptm::u2f(lo);
    if (levelLiteral(S, ptm::u2f(hi)) < k) return ptm::qnan();
    for (int s = 0; s < kBisectSteps; ++s) {   // L(lo) < k <= L(hi) throughout
        if (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (levelLiteral(S, ptm::u2f(mid)) >= k) hi = mid; else lo = mid;
        }
    }
    return ptm::u2f(hi);
}

// entry i of a table that is not a threshold or the flag: T[0], T[K + 1], T[K + 3], T[K + 4]
PTM_HD float fixedEntry(uint32_t i) { return i == 0u ? -ptm::inf() : ptm::qnan(); }

// T[k - 1], T[k] (2 <= k <= K) in the order a sorted table has them: non-decreasing, and no number behind a NaN
PTM_HD bool inOrder(float before, float at) { return at != at || at >= before; }

// the specification of the pixel: the number of k in 1 .. K with x >= T[k]
PTM_HD uint32_t levelCount(const float* T, uint32_t K, float x) {
    uint32_t n = 0u;
    for (uint32_t k = 1u; k <= K; ++k) n += (x >= T[k]) ? 1u : 0u;
    return n;
}

// the same number from a sorted table: the largest k in 0 .. K with x >= T[k] (none for a NaN: 0), K + 1 a power of two, 8 or 10 steps
PTM_HD uint32_t levelSearch(const float* T, uint32_t K, float x) {
    uint32_t k = 0u;
    for (uint32_t step = (K + 1u) >> 1; step != 0u; step >>= 1) k += (x >= T[k + step]) ? step : 0u;
    return k;
}

// the same number again, from any first guess k0 in 0 .. K: down while T[k] is above x or NaN, then up while T[k + 1] is not above x
// (T[0] = -inf stops the first loop for every number, k > 0 for a NaN; T[K + 1] = NaN stops the second)
PTM_HD uint32_t levelSettle(const float* T, uint32_t K, float x, uint32_t k0) {
    uint32_t k = k0;
    while (k > 0u && !(x >= T[k])) --k;
    while (k < K && x >= T[k + 1u]) ++k;
    return k;
}

PTM_HD uint32_t alphaOf(uint32_t K) { return K == 1023u ? 3u << 30 : 255u << 24; }
PTM_HD uint32_t shiftOf(uint32_t K) { return K == 1023u ? 10u : 8u; }

// the three channel inputs of a pixel from its unexposed means
PTM_HD void inputsOf(const float* mean, float exposure, const Rule& R, float* x) {
    const float er = mean[0] * exposure, eg = mean[1] * exposure, eb = mean[2] * exposure;
    if (R.luminance) {
        const float Y = ptm::fma(eb, kLumB, ptm::fma(eg, kLumG, er * kLumR));
        const float s = Y > 0.f ? ptm::div(curveOf(R.lum, Y), Y) : 0.f;
        x[0] = er * s, x[1] = eg * s, x[2] = eb * s;
    } else {
        x[0] = er, x[1] = eg, x[2] = eb;
    }
}

// a pixel shown from its three unexposed means and its weight; levelOf(x) is the level of a channel input
template <class LevelOf>
PTM_HD void showMeans(const float* mean, float weight, float exposure, const Rule& R, LevelOf&& levelOf, float* linear, uint32_t* px, float* hist) {
    float x[3];
    inputsOf(mean, exposure, R, x);
    uint32_t word = alphaOf(R.shown.K);
    for (int c = 0; c < 3; ++c) {
        linear[c] = mean[c];
        word |= levelOf(x[c]) << (shiftOf(R.shown.K) * (uint32_t)c);
        hist[c] = 255.f * valueOf(R.shown, x[c]);
    }
    linear[3] = hist[3] = weight;
    *px = word;
}

PTM_HD void showEmpty(const Rule& R, float* linear, uint32_t* px, float* hist) {
    linear[0] = linear[1] = linear[2] = linear[3] = 0.f;
    hist[0] = hist[1] = hist[2] = hist[3] = 0.f;
    *px = alphaOf(R.shown.K);
}

// one film entry resolved: the means of ptlin::resolve, ptspl::resolve (upSum null) or ptglare::resolve (upSum: up(u_1) at the pixel), shown
// through the tone rule. w: word 3 of the entry as those take it (the samples of a linear entry, the weight of a filtered one)
template <class LevelOf>
PTM_HD void resolve(u64 r, u64 g, u64 b, u64 w, bool splat, const u64* upSum, const ptglare::Rule* G, const ptlin::Scale& sc, const Rule& R,
                    LevelOf&& levelOf, float* linear, uint32_t* px, float* hist) {
    const u64 sum[3] = {r, g, b};
    float mean[3];
    if (upSum) {
        u64 shown[3];
        for (int c = 0; c < 3; ++c) {
            const u64 m = w == 0ull ? 0ull : (splat ? ptmeter::splatMean(sum[c], w) : ptmeter::linearMean(sum[c], w));
            shown[c] = ptglare::mixed(m, ptglare::glareOf(upSum[c], G->levels), *G);
        }
        if (w == 0ull && (shown[0] | shown[1] | shown[2]) == 0ull) return showEmpty(R, linear, px, hist);
        for (int c = 0; c < 3; ++c) mean[c] = (float)shown[c] * sc.down;
    } else {
        if (w == 0ull) return showEmpty(R, linear, px, hist);
        for (int c = 0; c < 3; ++c) mean[c] = splat ? ptspl::meanOf(sum[c], w, sc.down) : ptlin::meanOf(sum[c], w, sc.down);
    }
    showMeans(mean, splat ? (float)w * (1.f / ptspl::kOne) : (float)(uint32_t)w, sc.exposure, R, levelOf, linear, px, hist);
}

inline Stage stageOf(const ptss_tone_params& p, int curve) {
    Stage S;
    S.curve = curve;
    S.transfer = p.transfer;
    S.K = topOf(p.bits);
    S.rcpWhite2 = curve == PTSS_TONE_REINHARD ? ptm::div(1.f, p.white * p.white) : 0.f;
    const bool filmic = curve == PTSS_TONE_FILMIC;
    S.a = filmic ? p.filmic[0] : 0.f, S.b = filmic ? p.filmic[1] : 0.f, S.c = filmic ? p.filmic[2] : 0.f, S.d = filmic ? p.filmic[3] : 0.f;
    S.e = filmic ? p.filmic[4] : 1.f;
    return S;
}

inline Rule ruleOf(const ptss_tone_params& p) {
    const bool lum = (p.flags & PTSS_TONE_LUMINANCE) != 0u;
    return Rule{stageOf(p, lum ? PTSS_TONE_CLAMP : p.curve), stageOf(p, p.curve), lum ? 1u : 0u};
}

// what the tone calls refuse about their parameters, or nullptr. The last two conditions are what keeps a NaN out of the curve: the
// numerator and the denominator of either rational form do not fall as x grows, so a curve that is a number at +0 and at the saturation
// bound is one in between
inline const char* paramsError(const ptss_tone_params* p) {
    if (!p) return "tone params is null";
    if (p->structSize != sizeof(ptss_tone_params)) return "tone->structSize is not sizeof(ptss_tone_params)";
    if (p->curve != PTSS_TONE_CLAMP && p->curve != PTSS_TONE_REINHARD && p->curve != PTSS_TONE_FILMIC) return "unknown tone curve";
    if (p->transfer != PTSS_TRANSFER_GAMMA22 && p->transfer != PTSS_TRANSFER_SRGB) return "unknown transfer function";
    if (p->bits != 8 && p->bits != 10) return "bits must be 8 or 10";
    if (p->flags & ~PTSS_TONE_LUMINANCE) return "unknown tone flag";
    if (p->reserved != 0u) return "reserved must be 0";
    if (p->curve == PTSS_TONE_REINHARD) {
        if (!(p->white > 0.f && p->white <= 65536.f)) return "white must be in (0, 65536]";
        if (!(ptm::div(1.f, p->white * p->white) < ptm::inf())) return "1 / white^2 must be finite";
    }
    if (p->curve == PTSS_TONE_FILMIC) {
        for (int i = 0; i < 5; ++i)
            if (!(p->filmic[i] >= 0.f) || !(p->filmic[i] < ptm::inf())) return "filmic[] must be finite and not negative";
        if (!(p->filmic[4] > 0.f)) return "filmic[4] must be positive";
        const Stage S = stageOf(*p, p->curve);
        const float atZero = curveOf(S, 0.f), atBound = curveOf(S, kSaturate);
        if (atZero != atZero || atBound != atBound) return "filmic[] overflows at the saturation bound 2^40";
    }
    return nullptr;
}

// the whole table on the host, T[0 .. K + 4]; returns false where it is unsorted (T[K + 2] = 1)
inline bool buildTable(const ptss_tone_params& p, float* T) {
    const Stage S = ruleOf(p).shown;
    const uint32_t K = S.K;
    for (uint32_t k = 1u; k <= K; ++k) T[k] = thresholdOf(S, k);
    bool sorted = true;
    for (uint32_t k = 2u; k <= K; ++k) sorted = sorted && inOrder(T[k - 1u], T[k]);
    T[0] = fixedEntry(0u), T[K + 1u] = fixedEntry(K + 1u), T[K + 3u] = fixedEntry(K + 3u), T[K + 4u] = fixedEntry(K + 4u);
    T[K + 2u] = sorted ? 0.f : 1.f;
    return sorted;
}

}  // namespace pttone
#endif
