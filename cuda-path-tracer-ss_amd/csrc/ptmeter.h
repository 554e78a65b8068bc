// ptmeter.h — metering a linear or a filtered linear film (ptss_meter_linear / ptss_meter_splat / ptss_meter_exposure and the metered
// resolves): a pixel's integer mean, its luminance in fixed point, the luminance's bin of an eighth of a stop, and the
// exposure a histogram of such bins asks for, with temporal adaptation. PTM_HD over ptmath.h, ptlinear.h and ptsplat.h: the host build of
// this header (libptss_host.so, ptss_probe_meter_bin / ptss_probe_meter_linear / ptss_probe_meter_splat / ptss_probe_meter_exposure) is the
// specification, the kernels of ptss_meter.hip evaluate the same operations in the same order, and the two agree byte for byte.
//
// Everything in front of update()'s three float steps is integer work: a histogram is exact, order-free, and the same bytes for every
// grid shape and every split of a film into calls.
//
// The bound m <= 2^40 on both films. Linear film: every sample is at most 2^40 (ptlinear.h), so sum <= N * 2^40 and
// (sum + N / 2) / N <= 2^40 + 1/2, floored: 2^40. Filtered film: a tap adds (q * W + 32768) >> 16 <= q * W / 2^16 + 1/2 <= 2^24 * W + 1/2
// with q <= 2^40, and an integer that is at most 2^24 * W + 1/2 is at most 2^24 * W; summed, S <= 2^24 * Wt, hence
// (S * 2^16 + Wt / 2) / Wt <= 2^40 + 1/2, floored: 2^40. The weights sum to 256, so Y <= (256 * 2^40 + 128) >> 8 = 2^40 and a film the
// library filled never leaves bin 321. A film the caller filled with anything else cannot be kept from it: the products wrap like any
// unsigned integer and a luminance of 2^41 or more counts in the last bin, so no bin index ever leaves the histogram.
#ifndef PTSS_PTMETER_H
#define PTSS_PTMETER_H
#include "ptmath.h"
#include "ptlinear.h"
#include "ptsplat.h"

namespace ptmeter {

using ptlin::u64;

constexpr int kBins = PTSS_METER_BINS;   // bin 0: black; 1 + 8 e + sub for e = floor(log2 Y) in 0 .. 40
constexpr int kMaxLog2 = 40;
constexpr int kNoBin = -1;               // a pixel without samples is not metered
// the launch shape of the histogram kernels (ptss_meter.hip): a capped grid that strides the range. Every workgroup ends with one global
// atomic per non-zero bin, all workgroups on the same 329 words, so few large workgroups beat many small ones: one of sixteen waves per
// compute unit of a 256-CU device (measured against other shapes: DESIGN.md §3.31)
constexpr int kBlock = 1024;
constexpr int kGridCap = 256;

// the integer inside ptlin::meanOf and the one inside ptspl::meanOf, restated (the two films' resolves convert exactly these)
PTM_HD u64 linearMean(u64 sum, u64 N) { return (sum + N / 2ull) / N; }
PTM_HD u64 splatMean(u64 sum, u64 Wt) {
    const u64 a = sum / Wt, rem = sum % Wt;
    return (a << 16) + ((rem << 16) + Wt / 2ull) / Wt;
}

// Rec. 709 luminance with weights in 1/256 (54 + 183 + 19 = 256), rounded to nearest
PTM_HD u64 luminance(u64 mr, u64 mg, u64 mb) { return (54ull * mr + 183ull * mg + 19ull * mb + 128ull) >> 8; }

// an eighth of a stop per bin, linear in the mantissa inside an octave (at most 0.09 stop from a true logarithm; a design choice)
PTM_HD int binOfLuminance(u64 Y) {
    if (Y == 0ull) return 0;
    const int e = 63 - __builtin_clzll(Y);
    if (e > kMaxLog2) return kBins - 1;   // only a film the library did not fill gets here
    const int sub = (int)((e >= 3 ? Y >> (e - 3) : Y << (3 - e)) & 7ull);
    return 1 + 8 * e + sub;
}

PTM_HD int binOfLinear(u64 r, u64 g, u64 b, uint32_t samples) {
    if (samples == 0u) return kNoBin;
    const u64 N = (u64)samples;
    return binOfLuminance(luminance(linearMean(r, N), linearMean(g, N), linearMean(b, N)));
}

PTM_HD int binOfSplat(u64 r, u64 g, u64 b, u64 Wt) {
    if (Wt == 0ull) return kNoBin;
    return binOfLuminance(luminance(splatMean(r, Wt), splatMean(g, Wt), splatMean(b, Wt)));
}

// what update() takes of a ptss_meter_params and of the film's ptss_linear_params
struct Rule {
    float key, rate, minExposure, maxExposure;
    uint32_t lowPermille, highPermille;
    float scaleLog2;   // (float)scaleLog2: the film's fraction bits, taken off the mean logarithm
};

// Histogram -> exposure. T = the metered pixels that are not black; the ranks [lo, hi) are what the two percentile cuts leave of them, and
// the mean of the bin centres (in 1/16 stop: bin b's centre is 2 (b - 1) + 1) over those ranks is the scene's mean log2 luminance. All
// integers are unsigned 64-bit: T < 2^41, T * 999 < 2^51, sumLog < 2^51 — sums of integers, the same in any order, so the device may take
// them bin-parallel (ptss_meter.hip) — and three float steps follow, in expose(): one division, one exp, one fma.
PTM_HD u64 lowRank(u64 T, const Rule& R) { return T * (u64)R.lowPermille / 1000ull; }
PTM_HD u64 highRank(u64 T, const Rule& R) { return T - T * (u64)R.highPermille / 1000ull; }

// what bin b, holding the ranks [before, before + count), adds to sumLog: its overlap with [lo, hi) times its centre
PTM_HD u64 binLog(int b, u64 before, u64 count, u64 lo, u64 hi) {
    const u64 end = before + count;
    const u64 from = before > lo ? before : lo, to = end < hi ? end : hi;
    return to > from ? (to - from) * (u64)(2 * (b - 1) + 1) : 0ull;
}

// the state after an update whose integers are black, T, C = hi - lo (0 with T = 0) and sumLog
PTM_HD void expose(u64 black, u64 T, u64 C, u64 sumLog, const Rule& R, ptss_meter_state* s) {
    const bool fresh = s->updates == 0u;
    const float prev = fresh ? 1.f : s->exposure;
    float target = prev, exposure = prev, meanLog2 = fresh ? 0.f : s->meanLog2;
    if (T != 0ull) {   // (C >= 1: lowPermille + highPermille <= 999)
        meanLog2 = ptm::div((float)sumLog, (float)C * 16.f) - R.scaleLog2;
        target = ptm::clamp(R.key * ptm::exp(-meanLog2 * 0.69314718f), R.minExposure, R.maxExposure);
        exposure = fresh ? target : ptm::clamp(ptm::fma(target - prev, R.rate, prev), R.minExposure, R.maxExposure);
    }
    s->exposure = exposure;
    s->target = target;
    s->meanLog2 = meanLog2;
    s->updates = s->updates == 0xffffffffu ? s->updates : s->updates + 1u;
    s->metered = T;
    s->black = black;
    s->counted = C;
    s->sumLog = sumLog;
}

PTM_HD void update(const uint32_t* h, const Rule& R, ptss_meter_state* s) {
    u64 T = 0ull;
    for (int b = 1; b < kBins; ++b) T += (u64)h[b];
    u64 C = 0ull, sumLog = 0ull;
    if (T != 0ull) {
        const u64 lo = lowRank(T, R), hi = highRank(T, R);
        u64 before = 0ull;
        for (int b = 1; b < kBins; ++b) {
            sumLog += binLog(b, before, (u64)h[b], lo, hi);
            before += (u64)h[b];
        }
        C = hi - lo;
    }
    expose((u64)h[0], T, C, sumLog, R, s);
}

// what the meter calls refuse about their parameters, or nullptr
inline const char* paramsError(const ptss_meter_params* p) {
    if (!p) return "meter params is null";
    if (p->structSize != sizeof(ptss_meter_params)) return "params->structSize is not sizeof(ptss_meter_params)";
    if (!(p->key > 0.f) || !(p->key < ptm::inf())) return "key must be finite and positive";
    if (p->lowPermille > 999u || p->highPermille > 999u || p->lowPermille + p->highPermille > 999u)
        return "lowPermille + highPermille must not exceed 999";
    if (!(p->rate >= 0.f && p->rate <= 1.f)) return "rate must be in [0, 1]";
    if (!(p->minExposure >= 0.f) || !(p->maxExposure >= 0.f) || !(p->minExposure < ptm::inf()) || !(p->maxExposure < ptm::inf()))
        return "minExposure and maxExposure must be finite and not negative";
    if (p->minExposure > p->maxExposure) return "minExposure must not exceed maxExposure";
    if (p->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

inline Rule ruleOf(const ptss_meter_params& p, const ptss_linear_params& film) {
    return Rule{p.key, p.rate, p.minExposure, p.maxExposure, p.lowPermille, p.highPermille, (float)film.scaleLog2};
}

}  // namespace ptmeter
#endif
