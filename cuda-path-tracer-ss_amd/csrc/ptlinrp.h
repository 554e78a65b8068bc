// ptlinrp.h — carrying the two linear films across a camera move (ptss_reproject_linear): the previous pose's film,
// looked up through the first-hit features, SEEDS the new pose's film and moments once; from there the film is an ordinary film.
// PTM_HD over ptmath.h, ptcamera.h, ptreproject.h, ptlinear.h, ptmeter.h, ptlinstats.h and ptlindn.h: the host build of this header
// (libptss_host.so, ptss_probe_reproject_linear) is the specification, the kernels of ptss_linreproject.hip evaluate the same
// operations in the same order, compiled without contraction, and the two agree byte for byte.
//
// Pixel p = (x, y) of the `now` film with feature f_p:
//   1. (o, d) = ptcam::filmRay(now, x, y, 0.5, 0.5, ., .) with jitter 0 (the centre ray whose ptss_ray_features the caller passes).
//      hit (materialIdx >= 0): P = prevPoint_p of a motion row if given, else fma(d, depth_p, o); v = P - prev.position, r = |v|.
//      miss: v = d (the translation is ignored, §3.19).
//   2. l = rotate(conj(q_prev), v).
//      pinhole, thin lens (its centre rays pass through `position` with the pinhole's directions): rejected unless l.z zNear > 0;
//        fx = (l.x / (l.z s) + 0.5) W - 0.5, fy = (l.y / ((l.z s) aspect) + 0.5) H - 0.5           (§3.19's step 3)
//      equirect: rejected unless l is finite and not zero; lon = atan2(l.x, -l.z), lat = atan2(l.y, sqrt(l.x^2 + l.z^2));
//        fx = (lon / 2 pi + 0.5) W - 0.5, fy = (lat / pi + 0.5) H - 0.5; tap columns wrap (-1 is W - 1, W is 0), rows do not.
//        atan2(y, x), the quadrant rule: x = y = 0 -> 0. |x| >= |y|: a = atan(div(y, x)); x < 0: a + pi where y >= 0, a - pi
//        otherwise. |x| < |y|: (y > 0 ? pi / 2 : -pi / 2) - atan(div(x, y)). The quotient handed to ptm::atan lies in [-1, 1].
//      all: rejected unless -1 <= fx < W and -1 <= fy < H (which also keeps NaN from the conversions); x0 = floor(fx), tx = fx - x0
//      (y alike); taps (x0 + i, y0 + j) in the order (0,0) (1,0) (0,1) (1,1), b_q = (i ? tx : 1 - tx)(j ? ty : 1 - ty).
//   3. a tap counts iff it is inside the previous film (after the wrap), b_q > 0, its material equals f_p's (tested first), for
//      hits n_p . n_q >= cosNormal and |depth_q - r| <= depthTolerance r, and its film entry is not empty (ptldn::weightOf != 0).
//      Only then are the entry's divisions done and the moment row read.
//   4. over the counting taps, sums written around the FIRST counting tap (index 0): B = sum b_q, c_q = (float)m_q 2^-scaleLog2
//      (m_q = ptldn::meanOf), N_q = (float) the K of ptldn::countsOf;
//        h = c_0 + (sum b_q (c_q - c_0)) / B clamped per channel to the hull of the c_q;  w = N_0 + (sum b_q (N_q - N_0)) / B
//        K = min(rint(w), maxHistory)      (ties to even); B < minCoverage or K = 0: the pixel is empty
//      A previous film constant in mean or count comes back constant exactly: every difference is zero.
//   5. m' = ptlin::toFixed(h) per channel; linear film {m' K, m' K, m' K, samples = K, clamped = 0}, filtered film {.., weight = K << 16}.
//      ptmeter::linearMean(m' K, K) = (m' K + K / 2) / K = m' and splatMean(m' K, K << 16) = m' for m' <= 2^40, K < 2^23: m' K < 2^63,
//      m' K = a (K << 16) + rem with a = m' >> 16, rem = (m' & 65535) K < 2^39, and ((rem << 16) + (K << 15)) / (K << 16) = m' & 65535.
//   6. moments: a counting tap whose row has Nm_q >= 2 carries s2_q = se_q^2 Nm_q (se_q = ptls::standardError): the population
//      variance of its samples' luminance, taken as kMaxVariance = 2^80 where it is above that, infinite or NaN (only rows no film
//      holds get there): every s2_q is finite and in [0, 2^80]. s2 = the same anchored mean over the taps that carry one, with their
//      b_q, clamped to the hull of the s2_q, hence finite and in [0, 2^80] too. y' = ptmeter::luminance(m'). V = the float (float)K s2
//      as an integer: rounded to nearest even first where it is below ptlin::kIntegerFrom = 2^23; every float at or above 2^23 is an
//      integer already (so "exact from 2^24, rounded below" says the same). Q' = K y'^2 + V; the row is {y' K, Q' & (2^40 - 1),
//      Q' >> 40, K}: N Q - Sy^2 = K V, its standardError is sqrt(s2 / K).
//      The bound: m' <= clampMax 2^scaleLog2 <= 2^40 (ptlin::paramsError), so y' <= (256 2^40 + 128) >> 8 = 2^40 and K y'^2 < 2^103;
//      s2 <= 2^80 and K < 2^23 give V < 2^103; Q' < 2^104 and Q' >> 40 < 2^64. A consistent film never meets the clamp: the
//      population variance of values in [0, 2^40] is at most 2^78.
//      No tap carries one: the row is one pseudo-sample at the mean, {y', y'^2 & mask, y'^2 >> 40, 1}: "no information" to the
//      denoiser, below minSamples to the plan. An empty pixel is an all-zero row in both buffers.
#ifndef PTSS_PTLINRP_H
#define PTSS_PTLINRP_H
#include "ptmath.h"
#include "ptcamera.h"
#include "ptreproject.h"
#include "ptlinear.h"
#include "ptmeter.h"
#include "ptlinstats.h"
#include "ptlindn.h"

namespace ptlrp {
using namespace ptv;
using ptlin::u64;
using ptls::U128;

constexpr uint32_t kMaxHistoryLimit = (1u << 23) - 1u;
constexpr float kMaxVariance = 1208925819614629174706176.f;   // 2^80
constexpr float kHalfPi = 1.5707963267948966f;

// what became of a pixel (ptss_reproject_linear_info counts them)
constexpr int kSeeded = 0, kOffFilm = 1, kNoTap = 2;

struct Prev {   // the previous camera as the lookup reads it, evaluated on the host (prevOf)
    quat inverse;
    vec3 position;
    float zNear, s, aspect;
    float width, height;
    int kind, w, h;
};

struct Rule {   // the constants of a call
    float clampMax, up, down;   // the film's ptlin::Scale
    float cosNormal, depthTolerance, minCoverage, maxHistory;
};

struct Seed {   // what a pixel gets
    u64 film[4];
    u64 moment[4];
    int status;        // kSeeded, kOffFilm, kNoTap
    bool noVariance;   // seeded, moments asked for, no tap carried a variance
};

inline const char* paramsError(const ptss_reproject_linear_params* p) {
    if (!p) return "reproject params is null";
    if (p->structSize != (unsigned int)sizeof(ptss_reproject_linear_params))
        return "params->structSize is not sizeof(ptss_reproject_linear_params): start from ptss_default_reproject_linear_params";
    if (!(p->cosNormal >= -1.0f && p->cosNormal <= 1.0f)) return "cosNormal must be in [-1, 1]";
    if (!(p->depthTolerance >= 0.0f && p->depthTolerance < ptm::inf())) return "depthTolerance must be finite and not negative";
    if (!(p->minCoverage >= 0.0f && p->minCoverage <= 1.0f)) return "minCoverage must be in [0, 1]";
    if (p->maxHistory < 1u || p->maxHistory > kMaxHistoryLimit) return "maxHistory must be in [1, 2^23 - 1]";
    if (p->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// what the call refuses about one of its two cameras, or nullptr
inline const char* cameraError(const ptss_film_camera* f) {
    if (const char* what = ptcam::cameraError(f)) return what;
    if (f->width > ptspl::kMaxFilmSide || f->height > ptspl::kMaxFilmSide) return "a film's width and height must not exceed 2^22";
    if ((unsigned long long)f->width * (unsigned long long)f->height >= (1ull << 31)) return "a film's width * height must be below 2^31";
    return nullptr;
}

inline Rule ruleOf(const ptss_reproject_linear_params& p, const ptss_linear_params& film) {
    return Rule{film.clampMax, ptlin::pow2(film.scaleLog2), ptlin::pow2(-film.scaleLog2), p.cosNormal, p.depthTolerance, p.minCoverage,
                (float)p.maxHistory};
}

// whether [a, a + na) and [b, b + nb) share a byte: the refusal rule of the call and of the probe for their output ranges
inline bool rangesOverlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// what both refuse about their buffers (alignment aside), or nullptr; the cameras have passed cameraError
inline const char* buffersError(const ptss_film_camera* now, const void* featuresNow, const ptss_film_camera* prev, const void* featuresPrev,
                                const void* filmPrev, const void* momentsPrev, const void* filmOut, const void* momentsOut) {
    if (!featuresNow || !featuresPrev || !filmPrev || !filmOut) return "null features, previous film or output film";
    if ((momentsPrev == nullptr) != (momentsOut == nullptr)) return "dev_moments_prev and dev_moments_out must be given together or not at all";
    const size_t nowBytes = 32 * (size_t)now->width * (size_t)now->height, prevBytes = 32 * (size_t)prev->width * (size_t)prev->height;
    if (rangesOverlap(filmOut, nowBytes, filmPrev, prevBytes)) return "dev_film_out overlaps dev_film_prev";
    if (momentsOut && (rangesOverlap(filmOut, nowBytes, momentsPrev, prevBytes) || rangesOverlap(momentsOut, nowBytes, filmPrev, prevBytes) ||
                       rangesOverlap(momentsOut, nowBytes, momentsPrev, prevBytes) || rangesOverlap(momentsOut, nowBytes, filmOut, nowBytes)))
        return "the output film and moments overlap the previous film or moments, or each other";
    return nullptr;
}

// the `now` camera as filmRay takes it: the centre ray, whatever the caller's jitter says
inline ptcam::Film nowOf(const ptss_film_camera& f) {
    ptcam::Film F = ptcam::filmOf(f);
    F.jitter = 0;
    return F;
}

inline Prev prevOf(const ptss_film_camera& f) {
    const ptcam::Film F = ptcam::filmOf(f);
    const quat r = f.camera.rotation;
    return Prev{q4(r.w, -r.x, -r.y, -r.z), f.camera.position, f.camera.zNear, F.s, F.aspect, (float)f.width, (float)f.height, f.kind, f.width, f.height};
}

// the quadrant rule of the header comment; x and y finite
PTM_HD float atan2(float y, float x) {
    const float ax = ptm::abs(x), ay = ptm::abs(y);
    if (ax == 0.0f && ay == 0.0f) return 0.0f;
    if (ax >= ay) {
        const float a = ptm::atan(ptm::div(y, x));
        if (x < 0.0f) return y >= 0.0f ? a + ptm::kPi : a - ptm::kPi;
        return a;
    }
    return (y > 0.0f ? kHalfPi : -kHalfPi) - ptm::atan(ptm::div(x, y));
}

// step 2: where v lands on the previous film; false: rejected
PTM_HD bool project(const Prev& c, vec3 v, float& fx, float& fy) {
    const vec3 l = rotate(c.inverse, v);
    if (c.kind == PTSS_FILM_EQUIRECT) {
        if (!(ptrp::finite(l.x) && ptrp::finite(l.y) && ptrp::finite(l.z))) return false;
        if (l.x == 0.0f && l.y == 0.0f && l.z == 0.0f) return false;
        const float lon = atan2(l.x, -l.z);
        const float lat = atan2(l.y, ptm::sqrt(ptm::fma(l.z, l.z, l.x * l.x)));
        fx = (ptm::div(lon, ptcam::kTwoPi) + 0.5f) * c.width - 0.5f;
        fy = (ptm::div(lat, ptm::kPi) + 0.5f) * c.height - 0.5f;
    } else {
        if (!(l.z * c.zNear > 0.0f)) return false;
        const float zs = l.z * c.s;
        fx = (ptm::div(l.x, zs) + 0.5f) * c.width - 0.5f;
        fy = (ptm::div(l.y, zs * c.aspect) + 0.5f) * c.height - 0.5f;
    }
    return fx >= -1.0f && fx < c.width && fy >= -1.0f && fy < c.height;
}

// K as an integer-valued float: step 4's rounding and cap; 0 when the pixel stays empty
PTM_HD float historyCount(float w, float maxHistory) {
    const float k = ptm::min(__builtin_rintf(w), maxHistory);
    return k >= 1.0f ? k : 0.0f;
}

// a non-negative finite float below 2^104 as an integer: below 2^23 rounded to nearest even first
PTM_HD U128 toInteger(float f) {
    if (f < ptlin::kIntegerFrom) f = (f + ptlin::kIntegerFrom) - ptlin::kIntegerFrom;
    if (f < 9223372036854775808.f) return U128{(u64)f, 0ull};
    const uint32_t bits = ptm::f2u(f);
    const u64 mant = (u64)((bits & 0x7fffffu) | 0x800000u);
    const int shift = (int)(bits >> 23) - 150;   // 40 .. 80 here
    if (shift >= 64) return U128{0ull, mant << (shift - 64)};
    return U128{mant << shift, mant >> (64 - shift)};
}

// step 5: the film row of a pixel whose reprojected mean is h and whose history count is K >= 1; m[0..2]: the fixed-point means
PTM_HD void filmRow(vec3 h, u64 K, bool splat, const Rule& R, u64* m, u64* out) {
    uint32_t flag = 0u;
    m[0] = ptlin::toFixed(h.x, R.clampMax, R.up, &flag);
    m[1] = ptlin::toFixed(h.y, R.clampMax, R.up, &flag);
    m[2] = ptlin::toFixed(h.z, R.clampMax, R.up, &flag);
    out[0] = m[0] * K, out[1] = m[1] * K, out[2] = m[2] * K;
    out[3] = splat ? (K << 16) : K;
}

// step 6: the moment row beside it. has: some tap carried a variance, s2 then in [0, kMaxVariance]
PTM_HD void momentRow(const u64* m, u64 K, bool has, float s2, u64* out) {
    const ptls::Sample y = ptls::sampleOf(m[0], m[1], m[2]);
    if (!has) {
        out[0] = y.y, out[1] = y.lo, out[2] = y.hi, out[3] = 1ull;
        return;
    }
    const U128 sq = ptls::mul64(y.y, y.y);
    U128 Q = ptls::mul64(K, sq.lo);
    Q.hi += K * sq.hi;
    const U128 V = toInteger((float)K * s2);
    Q.lo += V.lo;
    Q.hi += V.hi + (Q.lo < V.lo ? 1ull : 0ull);
    out[0] = y.y * K;
    out[1] = Q.lo & ptls::kLoMask;
    out[2] = (Q.lo >> 40) | (Q.hi << 24);
    out[3] = K;
}

PTM_HD void emptySeed(Seed& s, int status) {
    s.film[0] = s.film[1] = s.film[2] = s.film[3] = 0ull;
    s.moment[0] = s.moment[1] = s.moment[2] = s.moment[3] = 0ull;
    s.status = status;
    s.noVariance = false;
}

// Pixel (x, y) of the `now` film. pointOf(o, d) -> vec3: the world point a HIT pixel is looked up at (called for hits only).
// materialAt(q) -> int, geometryAt(q) -> ptrp::Geometry: the PREVIOUS features; entryAt(q, u64[4]): the previous film's entry;
// momentAt(q, u64[4]): its moment row (Moments only). q = qy * prev.w + qx; each is called only for a tap inside the previous film,
// in that order, each behind the tests in front of it.
template <bool Moments, class PointOf, class MaterialAt, class GeometryAt, class EntryAt, class MomentAt>
PTM_HD void seedPixel(int x, int y, const ptdn::Feature& fp, const ptcam::Film& now, const Prev& prev, const Rule& R, bool splat, PointOf pointOf,
                      MaterialAt materialAt, GeometryAt geometryAt, EntryAt entryAt, MomentAt momentAt, Seed& out) {
    const ptss_ray_query ray = ptcam::filmRay(now, x, y, 0.5f, 0.5f, 0.0f, 0.0f);
    const bool hit = fp.materialIdx >= 0;
    vec3 v = ray.direction;
    float range = 0.0f;
    if (hit) {
        v = pointOf(ray.origin, ray.direction) - prev.position;
        range = length(v);
    }
    float fx, fy;
    if (!project(prev, v, fx, fy)) {
        emptySeed(out, kOffFilm);
        return;
    }
    const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
    const int x0 = (int)flx, y0 = (int)fly;
    const float tx = fx - flx, ty = fy - fly;
    const float tolerance = R.depthTolerance * range;
    const bool wrap = prev.kind == PTSS_FILM_EQUIRECT;
    vec3 c0 = v3(0, 0, 0), dsum = v3(0, 0, 0), lo = v3(0, 0, 0), hi = v3(0, 0, 0);
    float n0 = 0.0f, nsum = 0.0f, bsum = 0.0f;
    float s0 = 0.0f, ssum = 0.0f, sb = 0.0f, slo = 0.0f, shi = 0.0f;
    bool any = false, anyS = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const int i = k & 1, j = k >> 1;
        int qx = x0 + i;
        const int qy = y0 + j;
        if (wrap) qx = qx < 0 ? qx + prev.w : (qx >= prev.w ? qx - prev.w : qx);
        if (qx < 0 || qx >= prev.w || qy < 0 || qy >= prev.h) continue;
        const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
        if (!(b > 0.0f)) continue;
        const size_t q = (size_t)qy * (size_t)prev.w + (size_t)qx;
        if (materialAt(q) != fp.materialIdx) continue;
        if (hit) {
            const ptrp::Geometry g = geometryAt(q);
            if (!(dot(fp.normal, g.normal) >= R.cosNormal)) continue;
            if (!(ptm::abs(g.depth - range) <= tolerance)) continue;
        }
        u64 e[4];
        entryAt(q, e);
        const u64 wq = ptldn::weightOf(e[3], splat);
        if (wq == 0ull) continue;
        const vec3 c = v3((float)ptldn::meanOf(e[0], wq, splat) * R.down, (float)ptldn::meanOf(e[1], wq, splat) * R.down,
                          (float)ptldn::meanOf(e[2], wq, splat) * R.down);
        u64 Kq, clamped;
        ptldn::countsOf(e[3], splat, &Kq, &clamped);
        const float nq = (float)Kq;
        if (!any) {
            any = true;
            c0 = lo = hi = c;
            n0 = nq;
            bsum = b;
        } else {
            dsum = madd(c - c0, b, dsum);
            nsum = ptm::fma(nq - n0, b, nsum);
            bsum = bsum + b;
            lo = v3(ptm::min(lo.x, c.x), ptm::min(lo.y, c.y), ptm::min(lo.z, c.z));
            hi = v3(ptm::max(hi.x, c.x), ptm::max(hi.y, c.y), ptm::max(hi.z, c.z));
        }
        if constexpr (Moments) {
            u64 mq[4];
            momentAt(q, mq);
            if (mq[3] >= 2ull) {
                const float se = ptls::standardError(mq[0], mq[1], mq[2], mq[3]);
                const float raw = (se * se) * (float)mq[3];
                const float s2 = raw <= kMaxVariance ? raw : kMaxVariance;   // (an infinity or a NaN of rows no film holds ends here)
                if (!anyS) {
                    anyS = true;
                    s0 = slo = shi = s2;
                    sb = b;
                } else {
                    ssum = ptm::fma(s2 - s0, b, ssum);
                    sb = sb + b;
                    slo = ptm::min(slo, s2);
                    shi = ptm::max(shi, s2);
                }
            }
        }
    }
    if (!any || bsum < R.minCoverage) {
        emptySeed(out, kNoTap);
        return;
    }
    const float kf = historyCount(n0 + ptm::div(nsum, bsum), R.maxHistory);
    if (!(kf >= 1.0f)) {
        emptySeed(out, kNoTap);
        return;
    }
    const u64 K = (u64)kf;
    const vec3 mean = c0 + dsum / bsum;
    const vec3 h = v3(ptm::clamp(mean.x, lo.x, hi.x), ptm::clamp(mean.y, lo.y, hi.y), ptm::clamp(mean.z, lo.z, hi.z));
    u64 m[3];
    filmRow(h, K, splat, R, m, out.film);
    out.status = kSeeded;
    out.noVariance = false;
    out.moment[0] = out.moment[1] = out.moment[2] = out.moment[3] = 0ull;
    if constexpr (Moments) {
        float s2 = 0.0f;
        if (anyS) s2 = ptm::clamp(s0 + ptm::div(ssum, sb), slo, shi);   // every s2_q lies in [0, kMaxVariance]: finite sums, a finite hull
        momentRow(m, K, anyS, s2, out.moment);
        out.noVariance = !anyS;
    }
}

}  // namespace ptlrp
#endif
