// ptlinup.h — upsampling the two linear films in linear light (ptss_upsample_linear): a linear or a filtered linear film
// of W x H becomes a linear film of f W x f H, f = 1..4, guided by the first-hit features of both sizes, and every consumer of a linear
// film takes the result as it is. PTM_HD over ptupsample.h and ptlindn.h: the host build of this header (libptss_host.so,
// ptss_probe_upsample_linear) is the specification, the kernels of ptss_linupsample.hip evaluate the same operations in the same order,
// compiled without contraction, and the two agree byte for byte.
//
// A lo pixel q (loOf), once and not once per tap: w = ptldn::weightOf; w = 0: the pixel is empty, it has no colour and is never a tap.
// Otherwise m_q = ptldn::meanOf per channel, K_q from ptldn::countsOf (K_q >= 1, so K = 0 is the mark of an empty pixel), and
// c_q = (float)m_q * 2^-scaleLog2 (colourOf), the resolve's own steps.
//
// Hi pixel P = (X, Y) with hi feature F. ptup::axisOf on both axes gives the four taps q = (x0 + i, y0 + j), t = 2 j + i, with ptup's
// bilinear weight b_q and offsets; the depth slopes are ptdn::slope of the HI-RES depth, the exponent is ptdn::tapExponent with
// ptup::levelOf's constants. With PTSS_UPSAMPLE_LINEAR_WRAP_X tap columns wrap (-1 is W - 1, W is 0) and so do the slope's left and
// right hi-res neighbours, which then both always exist; rows never wrap. A tap counts iff it is inside the film (after the wrap), not
// empty, of F's material, and w_q = b_q exp(-e) > 0. The anchor a is the counted tap of the largest b_q, the lower index on a tie:
//     out = c_a + (sum_q w_q (c_q - c_a)) / sum_q w_q        in tap order through madd, the anchor's own zero included
// clamped per channel to the hull of the counted c_q; m' = ptlin::toFixed(out) — but in every channel in which all counted taps hold the
// same integer mean, m' is that integer: a constant film stays constant for every m, not only below 2^24, and f = 1 copies the means.
// The row is {m'_r K, m'_g K, m'_b K, samples = K, clamped = 0} with K = K_a: (m' K + K / 2) / K = m'.
// No tap counted: the nearest lo pixel (X div f, Y div f) — always one of the four taps and always inside — gives the row of its own
// integer means and K ("fallback"), or an all-zero row where it is empty ("empty").
//
// The choices this header makes where the formulas leave one:
//   - the four taps and the four depth neighbours are read UNCONDITIONALLY at coordinates wrapped, then clamped into their frames,
//     before the first test (as ptup::upsamplePixel does); what lies outside is decided afterwards
//   - the hull and the exact path look at counted taps only: a tap of weight 0 (b = 0 at f = 1, an underflow) has no say in either
//   - a K above 2^32 - 1 cannot arise: a linear entry's K is its 32-bit sample count, a filtered one's is capped at 2^23 - 1
//   - clamped of the output is 0 on both kinds: a clamped sample belongs to a lo pixel, not to the hi pixels made of it
#ifndef PTSS_PTLINUP_H
#define PTSS_PTLINUP_H
#include "ptupsample.h"
#include "ptlindn.h"

namespace ptlup {
using namespace ptv;
using ptlin::u64;

constexpr int kMaxFactor = ptup::kMaxFactor;
constexpr int kMaxSide = ptspl::kMaxFilmSide;
constexpr unsigned int kKnownFlags = PTSS_UPSAMPLE_LINEAR_WRAP_X;

// what became of a hi pixel (ptss_upsample_linear_info counts them)
constexpr int kFiltered = 0, kFallback = 1, kEmpty = 2;

struct Lo {   // a lo pixel as the taps read it
    u64 m[3];   // the integer means
    u64 K;      // the count of its output row; 0: the pixel is empty
};

struct Rule {   // the constants of a call, evaluated on the host and handed to the kernels as they are
    float clampMax, up, down;   // the film's ptlin::Scale
    ptdn::Level geo;            // ptup::levelOf
    int factor;
    int wrap;                   // PTSS_UPSAMPLE_LINEAR_WRAP_X
};

inline const char* paramsError(const ptss_upsample_linear_params* p) {
    if (!p) return "upsample params is null";
    if (p->structSize != (unsigned int)sizeof(ptss_upsample_linear_params))
        return "params->structSize is not sizeof(ptss_upsample_linear_params): start from ptss_default_upsample_linear_params";
    if (p->factor < 1 || p->factor > kMaxFactor) return "factor must be in [1, 4]";
    if (!(p->sigmaNormal > 0.0f && p->sigmaNormal < ptm::inf())) return "sigmaNormal must be finite and positive";
    if (!(p->sigmaDepth > 0.0f && p->sigmaDepth < ptm::inf())) return "sigmaDepth must be finite and positive";
    if (p->flags & ~kKnownFlags) return "unknown flag";
    if (p->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// what the call refuses about the sides (PTSS_ERANGE), or nullptr; factor has passed paramsError
inline const char* sidesError(int width, int height, int factor) {
    if (width < 1 || height < 1 || width > kMaxSide || height > kMaxSide) return "width and height must be in [1, 2^22]";
    const unsigned long long f = (unsigned long long)factor, hiW = f * (unsigned long long)width, hiH = f * (unsigned long long)height;
    if (hiW > (unsigned long long)kMaxSide || hiH > (unsigned long long)kMaxSide) return "factor * width and factor * height must not exceed 2^22";
    if (hiW * hiH >= (1ull << 31)) return "factor^2 * width * height must be below 2^31";
    return nullptr;
}

// whether the output film's range shares a byte with the input film's
inline bool rangesOverlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

inline Rule ruleOf(const ptss_upsample_linear_params& p, const ptss_linear_params& film) {
    ptss_upsample_params u;
    u.structSize = (unsigned int)sizeof(u);
    u.factor = p.factor;
    u.sigmaNormal = p.sigmaNormal;
    u.sigmaDepth = p.sigmaDepth;
    Rule R;
    R.clampMax = film.clampMax;
    R.up = ptlin::pow2(film.scaleLog2);
    R.down = ptlin::pow2(-film.scaleLog2);
    R.geo = ptup::levelOf(u);
    R.factor = p.factor;
    R.wrap = (p.flags & PTSS_UPSAMPLE_LINEAR_WRAP_X) ? 1 : 0;
    return R;
}

// a film entry (r, g, b, word3) as the taps read it: the wide divisions of a lo pixel, all of them
PTM_HD Lo loOf(u64 r, u64 g, u64 b, u64 word3, bool splat) {
    Lo o;
    const u64 w = ptldn::weightOf(word3, splat);
    if (w == 0ull) {
        o.m[0] = o.m[1] = o.m[2] = o.K = 0ull;
        return o;
    }
    o.m[0] = ptldn::meanOf(r, w, splat);
    o.m[1] = ptldn::meanOf(g, w, splat);
    o.m[2] = ptldn::meanOf(b, w, splat);
    u64 clamped;
    ptldn::countsOf(word3, splat, &o.K, &clamped);
    return o;
}

PTM_HD vec3 colourOf(const Lo& q, float down) { return v3((float)q.m[0] * down, (float)q.m[1] * down, (float)q.m[2] * down); }

// column x of a film `width` wide after the wrap (x in [-1, width]) and clamped into the film either way
PTM_HD int wrapped(int x, int width, bool wrap) { return wrap ? (x < 0 ? x + width : (x >= width ? x - width : x)) : x; }
PTM_HD int clamped(int x, int size) { return x < 0 ? 0 : (x >= size ? size - 1 : x); }

// the row of integer means m and count K
PTM_HD void rowOf(const u64* m, u64 K, u64* out) {
    out[0] = m[0] * K, out[1] = m[1] * K, out[2] = m[2] * K;
    out[3] = K;
}

// Hi pixel (X, Y) of a width x height LO film upsampled by R.factor; fp: its hi feature. Prepared: tapAt hands out Lo rows (the
// staged kernel divided once per lo pixel); otherwise film words, divided here, and only for the taps that count.
//   tapAt(tx, ty, cx, cy, u64[4])   the entry of lo pixel (cx, cy): {r, g, b, word3}, or (Prepared) {m_r, m_g, m_b, K}
//   featureAt(tx, ty, cx, cy)       -> ptdn::Feature of lo pixel (cx, cy)
//   depthAt(X, Y)                   -> the hi-res depth of hi pixel (X, Y)
// (tx, ty): the tap as axisOf gives it, x in [-1, width], y in [-1, height]; (cx, cy): the same wrapped and clamped into the film,
// which is the pixel to read. Returns kFiltered, kFallback or kEmpty; out: the four words of the hi pixel's ptss_linear_entry.
template <bool Prepared, class TapAt, class FeatureAt, class DepthAt>
PTM_HD int upsamplePixel(int X, int Y, int width, int height, const Rule& R, bool splat, const ptdn::Feature& fp, TapAt tapAt, FeatureAt featureAt,
                         DepthAt depthAt, u64* out) {
    const int f = R.factor;
    const bool wrap = R.wrap != 0;
    const ptup::Axis ax = ptup::axisOf(X, f), ay = ptup::axisOf(Y, f);
    // the loads: four taps and four depth neighbours, at coordinates inside their frames
    u64 word[4][4];
    ptdn::Feature fq[4];
    bool inside[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 4; ++t) {
        const int tx = ax.x0 + (t & 1), ty = ay.x0 + (t >> 1);
        const int qx = wrapped(tx, width, wrap);
        inside[t] = qx >= 0 && qx < width && ty >= 0 && ty < height;
        const int cx = clamped(qx, width), cy = clamped(ty, height);
        tapAt(tx, ty, cx, cy, word[t]);
        fq[t] = featureAt(tx, ty, cx, cy);
    }
    const int hiW = width * f, hiH = height * f;
    const bool l = wrap || X > 0, r = wrap || X + 1 < hiW, d = Y > 0, u = Y + 1 < hiH;
    const int Xl = X > 0 ? X - 1 : (wrap ? hiW - 1 : X), Xr = X + 1 < hiW ? X + 1 : (wrap ? 0 : X);
    const float zl = depthAt(Xl, Y), zr = depthAt(Xr, Y), zd = depthAt(X, d ? Y - 1 : Y), zu = depthAt(X, u ? Y + 1 : Y);
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (!Prepared) {
        // An empty statement that reads one register of every load above (ptup::upsamplePixel's): left alone, hipcc sinks a tap's
        // loads behind the tests that decide whether the tap counts, a wait before each. It changes no value.
        asm volatile("" ::"v"((uint32_t)word[0][3]), "v"((uint32_t)word[1][3]), "v"((uint32_t)word[2][3]), "v"((uint32_t)word[3][3]),
                     "v"((uint32_t)word[0][0]), "v"((uint32_t)word[1][0]), "v"((uint32_t)word[2][0]), "v"((uint32_t)word[3][0]), "v"(fq[0].depth),
                     "v"(fq[1].depth), "v"(fq[2].depth), "v"(fq[3].depth), "v"(fq[0].materialIdx), "v"(fq[1].materialIdx), "v"(fq[2].materialIdx),
                     "v"(fq[3].materialIdx), "v"(zl), "v"(zr), "v"(zd), "v"(zu));
    }
#endif

    const bool hit = fp.materialIdx >= 0;
    const float sx = ptdn::slope(fp.depth, l, zl, r, zr), sy = ptdn::slope(fp.depth, d, zd, u, zu);
    const float gx = hit ? sx : 0.0f, gy = hit ? sy : 0.0f;
    const vec3 zero = v3(0, 0, 0);
    // which taps count, their weights, the anchor
    float w[4], best = 0.0f;
    bool counts[4];
    int anchor = -1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 4; ++t) {
        const int i = t & 1, j = t >> 1;
        counts[t] = false;
        w[t] = 0.0f;
        if (!inside[t] || fq[t].materialIdx != fp.materialIdx) continue;
        if ((Prepared ? word[t][3] : ptldn::weightOf(word[t][3], splat)) == 0ull) continue;   // empty
        const float b = (i ? ax.f1 : 1.0f - ax.f1) * (j ? ay.f1 : 1.0f - ay.f1);
        const float offX = (float)(i ? 2 * f - ax.k : ax.k) * 0.5f, offY = (float)(j ? 2 * f - ay.k : ay.k) * 0.5f;
        const float e = ptdn::tapExponent(R.geo, zero, zero, fp, fq[t], gx, gy, offX, offY);
        const float wq = b * ptm::exp(-e);
        if (!(wq > 0.0f)) continue;   // an underflowed (or NaN) weight, or a bilinear weight of 0
        counts[t] = true;
        w[t] = wq;
        if (anchor < 0 || b > best) {
            anchor = t;
            best = b;
        }
    }
    // (an array is never indexed by a value the compiler cannot see: that would put it in scratch memory)
    auto loAt = [&](int t) -> Lo {
        return Prepared ? Lo{{word[t][0], word[t][1], word[t][2]}, word[t][3]} : loOf(word[t][0], word[t][1], word[t][2], word[t][3], splat);
    };
    if (anchor < 0) {
        // the nearest lo pixel: the tap on the side of the larger bilinear weight along each axis; always inside the film
        const int tn = (X / f - ax.x0) + 2 * (Y / f - ay.x0);
        u64 e[4] = {0ull, 0ull, 0ull, 0ull};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int t = 0; t < 4; ++t)
            if (t == tn)
                for (int k = 0; k < 4; ++k) e[k] = word[t][k];
        const Lo n = Prepared ? Lo{{e[0], e[1], e[2]}, e[3]} : loOf(e[0], e[1], e[2], e[3], splat);
        rowOf(n.m, n.K, out);   // K = 0: m = 0 too, the all-zero row
        return n.K == 0ull ? kEmpty : kFallback;
    }
    Lo q[4] = {}, qa = {};
    vec3 c[4] = {zero, zero, zero, zero}, ca = zero;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 4; ++t) {
        if (!counts[t]) continue;
        q[t] = loAt(t);
        c[t] = colourOf(q[t], R.down);
        if (t == anchor) {
            qa = q[t];
            ca = c[t];
        }
    }
    vec3 sum = zero, lo = ca, hi = ca;
    float wsum = 0.0f;
    bool same[3] = {true, true, true};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 4; ++t) {
        if (!counts[t]) continue;
        sum = madd(c[t] - ca, w[t], sum);
        wsum = wsum + w[t];
        lo = v3(ptm::min(lo.x, c[t].x), ptm::min(lo.y, c[t].y), ptm::min(lo.z, c[t].z));
        hi = v3(ptm::max(hi.x, c[t].x), ptm::max(hi.y, c[t].y), ptm::max(hi.z, c[t].z));
        for (int k = 0; k < 3; ++k) same[k] = same[k] && q[t].m[k] == qa.m[k];
    }
    const vec3 mean = ca + sum / wsum;
    const float o[3] = {ptm::clamp(mean.x, lo.x, hi.x), ptm::clamp(mean.y, lo.y, hi.y), ptm::clamp(mean.z, lo.z, hi.z)};
    uint32_t flag = 0u;
    u64 m[3];
    for (int k = 0; k < 3; ++k) m[k] = same[k] ? qa.m[k] : ptlin::toFixed(o[k], R.clampMax, R.up, &flag);
    rowOf(m, qa.K, out);
    return kFiltered;
}

}  // namespace ptlup
#endif
