// ptlindn.h — the denoiser of the two linear films (ptss_denoise_linear): an edge-avoiding A-trous filter in linear light
// whose luminance tolerance is each pixel's measured error, the standard error of its mean luminance from the film's exact moments
// (ptlinstats.h), and whose result is a linear film again. PTM_HD over ptmath.h, ptlinear.h, ptsplat.h, ptmeter.h, ptlinstats.h and
// ptdenoise.h: the host build of this header (libptss_host.so, ptss_probe_denoise_linear) is the specification, the kernels of
// ptss_lindenoise.hip evaluate the same operations in the same order, compiled without contraction, and the two agree byte for byte.
//
// Prepare, per pixel p. w = samples (a linear entry) or weight (a filtered one). w = 0: the pixel is empty — it has no colour, no pass
// takes it as a tap, its output row is all zero. Otherwise m = ptmeter::linearMean / splatMean per channel, c = (float)m * 2^-scaleLog2
// (the resolve's own steps), and from p's moment row (Sy, sqLo, sqHi, N), N the row's own count (on a filtered film the moments are kept by
// home pixel, §3.33, and that count applies): N >= 2: v = (ptls::standardError * 2^-scaleLog2)^2; N < 2: v = +inf, no information. A row
// of the colour/variance plane is {c.r, c.g, c.b, v}.
//
// One pass at level i (tap spacing s = 2^i) for a non-empty pixel p, taps q = p + s (i, j), i, j in -2..2, inside the frame, rows
// outward-in and i inside as ptdn::filterPixel walks them, empty taps skipped:
//     V_p   = the (1, 2, 1) x (1, 2, 1) average of v at spacing 1 around p over the taps in the frame and not empty, over the weights used
//     tol_p = max(sigmaLuminance * sqrt(V_p), 2^-scaleLog2)           one fixed-point step is the floor: never zero, never NaN
//     w_q   = h(i) h(j) exp(-(e_lum + e_geo))   if materialIdx_q == materialIdx_p, else 0
//     e_lum = |l(c_q) - l(c_p)| / tol_p                                sigmaLuminance does not halve per level: the variance shrinks instead
//     e_geo = e_normal + e_depth                                       ptdn::tapExponent itself, called with a zero colour term
//     c'    = c_p + (sum w_q (c_q - c_p)) / sum w_q,  w_p = h(0)^2 in the sum, clamped per channel to the hull of the taps with w_q > 0
//     v'    = (w_p^2 v_p + sum w_q^2 v_q) / (sum w)^2
// Finish, fused into the last pass: m' = ptlin::toFixed(c') per channel (clamped to [0, clampMax], round to nearest even at
// 2^scaleLog2), and the output row is {m'_r K, m'_g K, m'_b K, samples = K, clamped}: a linear entry whose integer mean is m' exactly
// ((m' K + K / 2) / K = m'). Linear film: K = samples, clamped carried over; filtered film: K = max(1, min((weight + 32768) >> 16,
// 2^23 - 1)), clamped = 0. m' K < 2^63 while K < 2^23; beyond that the product wraps, on both sides alike.
//
// The choices this header makes where the formulas leave one:
//   - an empty pixel's plane row is {0, 0, 0, -1}: a variance is never negative, so v < 0 is the mark, and every pass hands it on
//   - l(c) = fma(c.b, 19/256, fma(c.g, 183/256, c.r * (54/256))), everywhere
//   - V_p: acc = fma(k, v, acc) over rows j = -1..1, i inside, k = 1, 2 or 4; V_p = div(acc, sum of k). An infinite v makes V_p, tol_p
//     infinite and e_lum = div(x, inf) = 0: the pixel is filtered by its geometry alone
//   - the exponent is e_lum + (e_normal + e_depth), the bracket being ptdn::tapExponent's own sum; between two misses only e_lum counts
//   - v': w_q^2 is taken as w_q * w_q, and a tap whose w_q^2 is not > 0 (an underflowed square) adds nothing to v', so 0 * inf never
//     arises; an infinite v_p or v_q with w_q^2 > 0 makes v' infinite: inf stays inf
//   - levels = 0 runs prepare and finish only and finish takes the integer mean m itself, not its float: the output film's means equal
//     the input's for every m, not only below 2^24
#ifndef PTSS_PTLINDN_H
#define PTSS_PTLINDN_H
#include "ptmath.h"
#include "ptlinear.h"
#include "ptsplat.h"
#include "ptmeter.h"
#include "ptlinstats.h"
#include "ptdenoise.h"

namespace ptldn {
using namespace ptv;
using ptlin::u64;

constexpr int kMaxLevels = PTSS_DENOISE_MAX_LEVELS;
constexpr int kMaxSide = ptspl::kMaxFilmSide;
constexpr float kEmpty = -1.f;                    // v of an empty pixel
constexpr u64 kMaxSplatSamples = (1ull << 23) - 1ull;
// bytes of workspace per pixel: two colour/variance planes, the packed feature rows, the materials
constexpr size_t kPlaneBytes = 16, kFeatureBytes = 16, kMaterialBytes = 4;

struct Row {   // one row of a colour/variance plane
    vec3 c;
    float v;
};

// the constants of a call, evaluated on the host and handed to the kernels as they are
struct Rule {
    float clampMax, up, down;   // the film's ptlin::Scale
    float sigmaLuminance;
    float floorTol;             // 2^-scaleLog2
    ptdn::Level geo;            // ptdn::tapExponent's constants with invColor = 0; step is set per pass
};

PTM_HD bool isEmpty(const Row& r) { return r.v < 0.f; }
PTM_HD Row emptyRow() { return Row{v3(0.f, 0.f, 0.f), kEmpty}; }

PTM_HD float luminance(vec3 c) { return ptm::fma(c.z, 0.07421875f, ptm::fma(c.y, 0.71484375f, c.x * 0.2109375f)); }

// word 3 of a film entry as the weight w: the samples of a linear entry, the weight of a filtered one
PTM_HD u64 weightOf(u64 word3, bool splat) { return splat ? word3 : (word3 & 0xffffffffull); }

PTM_HD u64 meanOf(u64 sum, u64 w, bool splat) { return splat ? ptmeter::splatMean(sum, w) : ptmeter::linearMean(sum, w); }

// prepare: the plane row of a film entry (r, g, b, word3) with moment row (Sy, sqLo, sqHi, N)
PTM_HD Row prepare(u64 r, u64 g, u64 b, u64 word3, bool splat, u64 Sy, u64 sqLo, u64 sqHi, u64 N, const Rule& R) {
    const u64 w = weightOf(word3, splat);
    if (w == 0ull) return emptyRow();
    Row out;
    out.c = v3((float)meanOf(r, w, splat) * R.down, (float)meanOf(g, w, splat) * R.down, (float)meanOf(b, w, splat) * R.down);
    if (N >= 2ull) {
        const float se = ptls::standardError(Sy, sqLo, sqHi, N) * R.down;
        out.v = se * se;
    } else {
        out.v = ptm::inf();
    }
    return out;
}

// the K and the clamped count of an output row
PTM_HD void countsOf(u64 word3, bool splat, u64* K, u64* clamped) {
    if (splat) {
        const u64 k = (word3 + 32768ull) >> 16;
        *K = k < 1ull ? 1ull : (k > kMaxSplatSamples ? kMaxSplatSamples : k);
        *clamped = 0ull;
    } else {
        *K = word3 & 0xffffffffull;
        *clamped = word3 >> 32;
    }
}

// the output row (four 64-bit words of a ptss_linear_entry) of a non-empty pixel whose integer means are m[0..2]
PTM_HD void entryOf(const u64* m, u64 word3, bool splat, u64* out) {
    u64 K, clamped;
    countsOf(word3, splat, &K, &clamped);
    out[0] = m[0] * K, out[1] = m[1] * K, out[2] = m[2] * K;
    out[3] = K | (clamped << 32);
}

// finish of levels = 0: the integer means themselves
PTM_HD void finishMeans(u64 r, u64 g, u64 b, u64 word3, bool splat, u64* out) {
    const u64 w = weightOf(word3, splat);
    if (w == 0ull) {
        out[0] = out[1] = out[2] = out[3] = 0ull;
        return;
    }
    const u64 m[3] = {meanOf(r, w, splat), meanOf(g, w, splat), meanOf(b, w, splat)};
    entryOf(m, word3, splat, out);
}

// finish of the last pass: its row for a pixel whose film entry has `word3`
PTM_HD void finishRow(const Row& row, u64 word3, bool splat, const Rule& R, u64* out) {
    if (isEmpty(row)) {
        out[0] = out[1] = out[2] = out[3] = 0ull;
        return;
    }
    uint32_t flag = 0u;
    const u64 m[3] = {ptlin::toFixed(row.c.x, R.clampMax, R.up, &flag), ptlin::toFixed(row.c.y, R.clampMax, R.up, &flag),
                      ptlin::toFixed(row.c.z, R.clampMax, R.up, &flag)};
    entryOf(m, word3, splat, out);
}

// One pass for pixel (x, y) at tap spacing `step`. rowAt(qx, qy) -> Row, featureAt(qx, qy) -> ptdn::Feature, both only called for
// pixels inside the frame within 2 * step of (x, y) along each axis.
template <class RowAt, class FeatureAt>
PTM_HD Row filterPixel(int x, int y, int width, int height, int step, const Rule& R, RowAt rowAt, FeatureAt featureAt) {
    const Row rp = rowAt(x, y);
    if (isEmpty(rp)) return emptyRow();
    const ptdn::Feature fp = featureAt(x, y);
    ptdn::Level lv = R.geo;
    lv.step = step;
    float gx = 0.0f, gy = 0.0f;
    if (fp.materialIdx >= 0) {
        const bool l = x > 0, r = x + 1 < width, d = y > 0, u = y + 1 < height;
        gx = ptdn::slope(fp.depth, l, l ? featureAt(x - 1, y).depth : 0.0f, r, r ? featureAt(x + 1, y).depth : 0.0f);
        gy = ptdn::slope(fp.depth, d, d ? featureAt(x, y - 1).depth : 0.0f, u, u ? featureAt(x, y + 1).depth : 0.0f);
    }
    // V_p
    float acc = 0.0f, used = 0.0f;
    for (int j = -1; j <= 1; ++j) {
        const int qy = y + j;
        if (qy < 0 || qy >= height) continue;
        for (int i = -1; i <= 1; ++i) {
            const int qx = x + i;
            if (qx < 0 || qx >= width) continue;
            const float vq = (i == 0 && j == 0) ? rp.v : rowAt(qx, qy).v;
            if (vq < 0.f) continue;
            const float k = (float)((i == 0 ? 2 : 1) * (j == 0 ? 2 : 1));
            acc = ptm::fma(k, vq, acc);
            used = used + k;
        }
    }
    const float tol = ptm::max(R.sigmaLuminance * ptm::sqrt(ptm::div(acc, used)), R.floorTol);
    const float lp = luminance(rp.c);
    const vec3 cp = rp.c, zero = v3(0.f, 0.f, 0.f);
    vec3 sum = zero, lo = cp, hi = cp;
    float wsum = ptdn::spline(0) * ptdn::spline(0);
    float vsum = (wsum * wsum) * rp.v;
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * step;
        if (qy < 0 || qy >= height) continue;
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * step;
            if (qx < 0 || qx >= width || (i == 0 && j == 0)) continue;
            const ptdn::Feature fq = featureAt(qx, qy);
            if (fq.materialIdx != fp.materialIdx) continue;
            const Row rq = rowAt(qx, qy);
            if (isEmpty(rq)) continue;
            const float eLum = ptm::div(ptm::abs(luminance(rq.c) - lp), tol);
            const float eGeo = ptdn::tapExponent(lv, zero, zero, fp, fq, gx, gy, (float)((i < 0 ? -i : i) * step), (float)((j < 0 ? -j : j) * step));
            const float w = (ptdn::spline(i) * ptdn::spline(j)) * ptm::exp(-(eLum + eGeo));
            if (!(w > 0.0f)) continue;   // an underflowed (or NaN) weight contributes nothing, not even to the clamp
            sum = madd(rq.c - cp, w, sum);
            wsum = wsum + w;
            lo = v3(ptm::min(lo.x, rq.c.x), ptm::min(lo.y, rq.c.y), ptm::min(lo.z, rq.c.z));
            hi = v3(ptm::max(hi.x, rq.c.x), ptm::max(hi.y, rq.c.y), ptm::max(hi.z, rq.c.z));
            const float w2 = w * w;
            if (w2 > 0.0f) vsum = ptm::fma(w2, rq.v, vsum);
        }
    }
    const vec3 out = cp + sum / wsum;
    Row res;
    res.c = v3(ptm::clamp(out.x, lo.x, hi.x), ptm::clamp(out.y, lo.y, hi.y), ptm::clamp(out.z, lo.z, hi.z));
    res.v = ptm::div(vsum, wsum * wsum);
    return res;
}

// where the parts of a workspace over P pixels lie, in bytes from its start (each a multiple of 16): plane 0, plane 1, the feature
// rows {normal, depth}, the materials; returns the size
inline size_t workspaceLayout(size_t P, size_t off[4]) {
    const size_t plane = P * kPlaneBytes;
    off[0] = 0;
    off[1] = plane;
    off[2] = 2 * plane;
    off[3] = 2 * plane + P * kFeatureBytes;
    return (off[3] + P * kMaterialBytes + 15) & ~(size_t)15;
}

// the plane pass i (0-based) reads; it writes the other. Prepare writes plane 0
inline int sourcePlane(int pass) { return pass & 1; }

// what ptss_denoise_linear refuses about its own parameters (PTSS_EINVAL), or nullptr
inline const char* paramsError(const ptss_denoise_linear_params* p) {
    if (!p) return "denoise params is null";
    if (p->structSize != sizeof(ptss_denoise_linear_params)) return "denoise->structSize is not sizeof(ptss_denoise_linear_params)";
    if (p->levels < 0 || p->levels > kMaxLevels) return "levels must be in [0, 6]";
    const float s[3] = {p->sigmaLuminance, p->sigmaNormal, p->sigmaDepth};
    for (int k = 0; k < 3; ++k)
        if (!(s[k] > 0.f) || !(s[k] < ptm::inf())) return "sigmaLuminance, sigmaNormal and sigmaDepth must be finite and positive";
    if (p->reserved[0] != 0u || p->reserved[1] != 0u || p->reserved[2] != 0u) return "reserved must be 0";
    return nullptr;
}

// what it refuses about the film's sides (PTSS_ERANGE), or nullptr: ptss_glare_build's limits
inline const char* sidesError(int width, int height) {
    if (width < 1 || height < 1 || width > kMaxSide || height > kMaxSide) return "width and height must be in [1, 2^22]";
    if ((unsigned long long)width * (unsigned long long)height >= (1ull << 31)) return "width * height must be below 2^31";
    return nullptr;
}

inline Rule ruleOf(const ptss_denoise_linear_params& p, const ptss_linear_params& film) {
    Rule R;
    R.clampMax = film.clampMax;
    R.up = ptlin::pow2(film.scaleLog2);
    R.down = ptlin::pow2(-film.scaleLog2);
    R.sigmaLuminance = p.sigmaLuminance;
    R.floorTol = R.down;
    R.geo.step = 1;
    R.geo.radius = 2;
    R.geo.invColor = 0.0f;
    R.geo.invNormal = 1.0f / p.sigmaNormal;
    R.geo.sigmaDepth = p.sigmaDepth;
    return R;
}

}  // namespace ptldn
#endif
