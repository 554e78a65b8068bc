// ptspecular.h — the arithmetic of ptss_render_features_specular, written once for the gfx950 kernel (ptss_kernels.hip
// specularFeatureKernel) and for the host probe (host_capi.cpp ptss_probe_specular_step; tests/test_specular_cpu.py). Everything is
// float32 built from ptmath.h operations in the order written here, compiled without contraction on both sides, so the two builds
// agree bit for bit.
//
// The centre ray of a pixel is carried through the DELTA lobes of the surfaces it meets — perfect reflection, refraction — to the
// first surface that is not one; the features are taken there. Which lobe a hit continues with is decided from the material alone,
// with no random draw (scatter(), ptshade.h, picks a lobe by a uniform; here a material has one class):
//   TERMINAL   (flags & 0x03) == 0x03 (Cook-Torrance: its only specular lobe is a Beckmann distribution), or diffAvg > 0
//   TRANSMIT   otherwise, refrAvg > 0
//   MIRROR     otherwise, specAvg > 0 and specularExponent == +inf
//   TERMINAL   otherwise (a glossy Phong lobe only, or an absorber)
//
// The step at a hit (point, normal) of ray (o, d) is scatter()'s, line for line (ptshade.h; the reference's lines in brackets):
//   here                                            scatter()
//   cosI = dot(-d, normal)                          bounceTile's `cosI = dot(-ray.d, normal)`, scatter's argument
//   if (cosI > 0) n2 = ior, n1 = 1                  `if (cosI > 0) { n2 = mMisc.y; n1 = 1.0f; }`               [:474-494]
//   else cosI = -cosI, n1 = ior, n2 = 1             `else { cosI = -cosI; n1 = mMisc.y; n2 = 1.0f; }`
//   reflect(): d' = d - (2 * (-cosI)) * normal      `ray.d = ray.d - (2 * (-cosI)) * normal`                   [reflRay :496-503]
//              o' = point + (normal * kRayBump)     `ray.o = point + (normal * ptm::kRayBump)`
//   n = div(n1, n2)                                 `n = ptm::div(n1, n2)`                                     [:491-493]
//   sinT2 = n * n * (1 - cosI * cosI)               `sinT2 = n * n * (1.0f - cosI * cosI)`
//   !(sinT2 > 1):                                   scatter's refraction lobe takes refrRay unless `sinT2 > 1.0f` [refrRay :516-531]
//     cosT = sqrt(1 - sinT2)                        `cosT = ptm::sqrt(1.0f - sinT2)`
//     w_o = normalize(n * d + (n * cosI - cosT) * normal)   `w_o = normalize(n * ray.d + (n * cosI - cosT) * normal)`
//     o' = point + (w_o * kRayBump), d' = w_o       `ray.o = point + (w_o * ptm::kRayBump); ray.d = w_o`
//   sinT2 > 1 (total internal reflection):          fresnelReflective stays 1, the refraction lobe has weight 0 and ends the path:
//     specAvg > 0: reflect(), else terminal         the specular lobe (`mSpecular.w > 0.0f`) is the only one scatter() can take, and
//                                                   it takes reflRay whatever the exponent (a finite one then perturbs the direction
//                                                   with a random draw, which a centre ray does not have)
// The chain continues only if all three components of d' are finite.
#pragma once
#include "ptmath.h"

namespace ptsp {
using namespace ptv;

constexpr int kMaxSteps = 8;   // ptss_render_features_specular's maxSteps: 0 .. kMaxSteps

enum Class : int { kTerminal = 0, kTransmit = 1, kMirror = 2 };

struct Material {   // the words of a material the step reads (scatter()'s mDiffuse.w, mSpecular.w, refrAvg, mMisc.x, mMisc.y, flags)
    float diffAvg, specAvg, refrAvg, specularExponent, indexOfRefraction;
    int flags;
};

PTM_HD Class classify(const Material& m) {
    if ((m.flags & PTSS_MAT_FLAG_COOK_TORRANCE) == PTSS_MAT_FLAG_COOK_TORRANCE || m.diffAvg > 0.0f) return kTerminal;
    if (m.refrAvg > 0.0f) return kTransmit;
    if (m.specAvg > 0.0f && m.specularExponent == ptm::inf()) return kMirror;
    return kTerminal;
}

struct Step {
    bool follows;
    vec3 o, d;   // the continued ray (meaningful when follows)
};

PTM_HD bool finite3(vec3 v) { return ptm::abs(v.x) < ptm::inf() && ptm::abs(v.y) < ptm::inf() && ptm::abs(v.z) < ptm::inf(); }   // (false for NaN)

PTM_HD Step step(const Material& m, vec3 d, vec3 point, vec3 normal) {
    Step s{false, v3(0, 0, 0), v3(0, 0, 0)};
    const Class cls = classify(m);
    if (cls == kTerminal) return s;
    float cosI = dot(-d, normal);
    float n1, n2;
    if (cosI > 0) {
        n2 = m.indexOfRefraction;
        n1 = 1.0f;
    } else {
        cosI = -cosI;
        n1 = m.indexOfRefraction;
        n2 = 1.0f;
    }
    bool reflects = cls == kMirror;
    if (cls == kTransmit) {
        const float n = ptm::div(n1, n2);
        const float sinT2 = n * n * (1.0f - cosI * cosI);
        if (!(sinT2 > 1.0f)) {   // refrRay
            const float cosT = ptm::sqrt(1.0f - sinT2);
            const vec3 w_o = normalize(n * d + (n * cosI - cosT) * normal);
            s.o = point + (w_o * ptm::kRayBump);
            s.d = w_o;
        } else {
            if (!(m.specAvg > 0.0f)) return s;   // total internal reflection without a specular lobe: the path ends
            reflects = true;
        }
    }
    if (reflects) {   // reflRay
        s.d = d - (2 * (-cosI)) * normal;
        s.o = point + (normal * ptm::kRayBump);
    }
    s.follows = finite3(s.d);
    return s;
}

// The factor by which the link step() follows multiplies the radiance that arrives along it (ptss_intersect_chain's throughput;
// host_capi.cpp ptss_probe_specular_link): the probability with which scatter() picks the followed lobe times the
// weight scatter() returns for it, so that a chain's product is the expectation of the reference's estimator restricted to the chain.
// scatter()'s own expressions in scatter()'s order (ptshade.h; ptm::div where scatter() may take a proven fast path to the same
// bits); cosI, n1 and n2 flipped as step() flips them:
//   F = 1; the Snell / Fresnel terms only where scatter() reads them:
//   (specAvg > 0 && !(flags & PURE_REFLECTION)) || refrAvg > 0:
//     n = div(n1, n2), sinT2 = n * n * (1 - cosI * cosI)
//     !(sinT2 > 1): cosT = sqrt(1 - sinT2), r_s = div(n1 cosI - n2 cosT, n1 cosI + n2 cosT), r_p = div(n2 cosI - n1 cosT,
//                   n2 cosI + n1 cosT), F = (r_s r_s + r_p r_p) * 0.5
//   a reflected link (MIRROR, or TRANSMIT in total internal reflection): p = (flags & PURE_REFLECTION) ? specAvg : specAvg * F,
//                                                                      factor = specularColor * p
//   a refracted link:                                                  p = refrAvg * (1 - F), factor = (p, p, p)
// Meaningful only for a link that follows (step().follows); specularColor: the material's (scatter()'s xyz(mSpecular)), an argument
// of its own so that Material stays what step() reads.
PTM_HD vec3 linkFactor(const Material& m, vec3 specularColor, vec3 d, vec3 normal) {
    const Class cls = classify(m);
    float cosI = dot(-d, normal);
    float n1, n2;
    if (cosI > 0) {
        n2 = m.indexOfRefraction;
        n1 = 1.0f;
    } else {
        cosI = -cosI;
        n1 = m.indexOfRefraction;
        n2 = 1.0f;
    }
    float F = 1.0f, sinT2 = 0.0f;
    if ((m.specAvg > 0.0f && !(m.flags & PTSS_MAT_FLAG_PURE_REFLECTION)) || m.refrAvg > 0.0f) {
        const float n = ptm::div(n1, n2);
        sinT2 = n * n * (1.0f - cosI * cosI);
        if (!(sinT2 > 1.0f)) {
            const float cosT = ptm::sqrt(1.0f - sinT2);
            const float r_s = ptm::div(n1 * cosI - n2 * cosT, n1 * cosI + n2 * cosT);
            const float r_p = ptm::div(n2 * cosI - n1 * cosT, n2 * cosI + n1 * cosT);
            F = (r_s * r_s + r_p * r_p) * 0.5f;
        }
    }
    if (cls == kMirror || (cls == kTransmit && sinT2 > 1.0f)) {
        const float p = (m.flags & PTSS_MAT_FLAG_PURE_REFLECTION) ? m.specAvg : m.specAvg * F;
        return specularColor * p;
    }
    const float p = m.refrAvg * (1.0f - F);
    return v3(p, p, p);
}

}  // namespace ptsp
