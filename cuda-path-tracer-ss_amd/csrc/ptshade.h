// ptshade.h — layer 4 of the device code of ptss_kernels.hip: what happens to a path at a surface and at its end. One light's
// Lambert term (CudaTracer.cu:360-366), computeIndirectRadianceAndScatter with its three samplers (CudaTracer.cu:208-318, :533-585),
// writeToPixelsKernel for one finished path (CudaTracer.cu:63-104) with the random stream's home record, and the whole-frame loop
// guard of frame lanes (CudaTracer.cu:622).
#pragma once
#include "ptaccel.h"   // ptss_diag.h's hooks
#include "ptquant.h"
#include "ptraypool.h"

namespace ptss {
namespace {

// The geometry of one light sample, the head of lineOfSight (CudaTracer.cu:423-432): distance2 = |offset|^2, distance = sqrt(distance2),
// w_i = offset / distance. When every active lane's distance2 lies in the light-sample window [kLightD2Lo, kLightD2Hi) of ptmath.h
// and every offset component has a magnitude of at least 2^-60, the root and the three divisions of w_i run without their own range
// guards (2 + 8 compares); addLambertTerm tests the same window again for the divisor 4 pi distance2 (one compare, instead of a verdict
// held in scalar registers across the shadow passes):
//   * the window's ends are derived in ptmath.h from the three operations' ranges;
//   * the numerators need no upper test: distance2 = fma(z, z, fma(y, y, x * x)) is a sum of non-negative terms rounded three times,
//     so distance2 >= c^2 (1 - 2^-24)^3 for each component c (c^2 cannot underflow when |c| >= 2^-60), and distance2 < kLightD2Hi
//     < 2^57 gives |c| < 2^28.5 (1 + 2^-22) < 2^60;
//   * their lower tests are one v_min3_f32 of the magnitudes and one compare (a NaN component makes distance2 NaN, which fails the
//     window).
// A wave that fails the test runs the guarded operations, exactly as before; inside the window both give the same bits.
__device__ __forceinline__ void lightSample(vec3 offset, float& distance2, float& distance, vec3& w_i) {
    distance2 = dot(offset, offset);
    const float least = __builtin_fminf(__builtin_fminf(ptm::abs(offset.x), ptm::abs(offset.y)), ptm::abs(offset.z));
    PTSS_DIAG_GUARD_LIGHT(offset, distance2, least);
    if (__builtin_expect(ptm::every_lane(ptm::in_light_window(distance2), least >= ptm::kDivLo), 1)) {
        distance = ptm::sqrt_in_range(distance2);
        ptm::div3_in_range(offset.x, offset.y, offset.z, distance, w_i.x, w_i.y, w_i.z);
    } else {
        distance = ptm::sqrt(distance2);
        w_i = offset / distance;
    }
}

// one light's Lambert term, CudaTracer.cu:360-366 / :379-385. powersProven: the scene's kGuardLightPowers. With it and every active
// lane's distance2 in the light-sample window, the divisor 4 pi distance2 is in [2^-60, 2^60) and positive, every power component is
// +0 or in range (ptm::fast_numerator says why +0 may stay), and the three quotients need no guard.
__device__ __forceinline__ void addLambertTerm(vec3& radiance, float cosI, vec3 power, float distance2,
                                               float4 diffuse /* colour, diffAvg */, bool powersProven) {
    const float divisor = (float)(ptm::kFourPi * distance2);
    vec3 L_i;
    PTSS_DIAG_GUARD_POWER(power, divisor);
    if (powersProven && ptm::every_lane(ptm::in_light_window(distance2))) ptm::div3_in_range(power.x, power.y, power.z, divisor, L_i.x, L_i.y, L_i.z);
    else L_i = power / divisor;
    radiance.x += cosI * L_i.x * diffuse.x * diffuse.w * ptm::kInvPi;
    radiance.y += cosI * L_i.y * diffuse.y * diffuse.w * ptm::kInvPi;
    radiance.z += cosI * L_i.z * diffuse.z * diffuse.w * ptm::kInvPi;
}

// CudaTracer.cu:579-585
__device__ __forceinline__ quat rotateVectorToVector(vec3 source, vec3 target) {
    const vec3 axis = cross(source, target);
    return normalize(q4(1.0f + dot(source, target), axis.x, axis.y, axis.z));
}

// ---- computeIndirectRadianceAndScatter, CudaTracer.cu:208-318 ---------------------------------
// The three random-direction samplers of the reference (Lambert :533-545, Phong :547-559, Beckmann :561-577) all
// draw two uniforms and end the same way: a vector (a*cos(az), y, a*sin(az)) about +Y, rotated onto the lobe axis by
// rotateVectorToVector (:579-585). With 64 incoherent rays nearly every wave holds lanes of all three kinds, so the
// lobe CHOICE runs divergently (it is cheap) and the draws + sincos + rotation run ONCE, for all sampling lanes
// together; each lane performs exactly the operations, in the order, that its own sampler performs in the
// reference (the draws keep their order: Lambert/Phong use the first for the azimuth and the second for the
// elevation, Beckmann the first for the elevation and the second for the azimuth).
enum LobeKind { kLobeNone = 0, kLobeLambert = 1, kLobePhong = 2, kLobeBeckmann = 3 };

// guardFlags: FrameBuffers::guardFlags — the scene constants among the operands below whose range guard was settled at ptss_create.
__device__ __forceinline__ vec3 scatter(const float4* mat, RayRegs& ray, vec3 point, vec3 normal, float cosI, uint32_t guardFlags) {
    const float4 mDiffuse = mat[0];   // diffuseColor, diffAvg
    const float4 mSpecular = mat[1];  // specularColor, specAvg
    const float4 mMisc = mat[4];      // specularExponent, indexOfRefraction, flags
    const float refrAvg = mat[2].w;
    const int flags = (int)asU(mMisc.z);

    float r = ptrng::uniform(ray.rng);
    PTSS_DIAG_SCATTER(0, true);  // waves (and lanes) in scatter at all

    int kind = kLobeNone;
    bool decided = false;
    vec3 axis = normal;
    vec3 result = v3(0, 0, 0);
    const vec3 incident = ray.d;

    if (mDiffuse.w > 0.0f) {
        r -= mDiffuse.w;
        if (r < 0.0f) {  // randomDirectionLambert about the normal
            ray.o = point + ptm::kRayBump * normal;
            kind = kLobeLambert;
            decided = true;
            result = xyz(mDiffuse);
        }
    }

    PTSS_DIAG_SCATTER(1, !decided);  // the non-Lambert block
    if (!decided) {
        // computeSinT2AndRefractiveIndexes :474-494 (flips cosI when inside)
        float n1, n2;
        if (cosI > 0) {
            n2 = mMisc.y;
            n1 = 1.0f;
        } else {
            cosI = -cosI;
            n1 = mMisc.y;
            n2 = 1.0f;
        }
        // The Snell / Fresnel terms (two square roots' worth and three divisions) feed only the Fresnel-weighted specular
        // lobe (:248-249) and the refraction lobe (:300-311). A material with the pure-reflection bit (mirrors AND every
        // Cook-Torrance material, 0x03 & 0x01) and no refraction never reads them: its lanes skip the block, and a wave
        // without glass skips it altogether. (cosI's flip above is kept: reflRay uses it.)
        const bool readsFresnel = (mSpecular.w > 0.0f && !(flags & PTSS_MAT_FLAG_PURE_REFLECTION)) || refrAvg > 0.0f;
        float n = 0.0f, sinT2 = 0.0f;
        float fresnelReflective = 1.0f;
        PTSS_DIAG_SCATTER(2, readsFresnel);  // Snell / Fresnel terms
        if (readsFresnel) {
            PTSS_DIAG_GUARD_DIV(7, n1, n2);
            // computeSinT2AndRefractiveIndexes :491-493. One operand is 1, the other the material's index: kGuardRefraction settles both
            n = (guardFlags & kGuardRefraction) ? ptm::div_in_range_operands(n1, n2) : ptm::div(n1, n2);
            sinT2 = n * n * (1.0f - cosI * cosI);
        }
        if (readsFresnel && !(sinT2 > 1.0f)) {   // computeFresnelForReflectance :457-472
            const float cosT = ptm::sqrt(1.0f - sinT2);
            const float r_s = ptm::div(n1 * cosI - n2 * cosT, n1 * cosI + n2 * cosT);
            const float r_p = ptm::div(n2 * cosI - n1 * cosT, n2 * cosI + n1 * cosT);
            fresnelReflective = (r_s * r_s + r_p * r_p) * 0.5f;
        }

        if (mSpecular.w > 0.0f) {
            if (flags & PTSS_MAT_FLAG_PURE_REFLECTION)
                r -= mSpecular.w;
            else
                r -= mSpecular.w * fresnelReflective;

            if (r < 0.0f) {
                decided = true;
                if (flags & PTSS_MAT_FLAG_COOK_TORRANCE) {
                    kind = kLobeBeckmann;  // micro-normal about the surface normal; the reflection follows below
                } else {
                    // reflRay(ray, surfel, cosI) :496-503
                    ray.d = ray.d - (2 * (-cosI)) * normal;
                    ray.o = point + (normal * ptm::kRayBump);
                    if (mMisc.x != ptm::inf()) {  // randomDirectionPhong about the mirror direction
                        kind = kLobePhong;
                        axis = ray.d;
                    }
                    result = xyz(mSpecular);
                }
            }
        }

        if (!decided && refrAvg > 0.0f) {
            const float fresnelRefractive = 1.0f - fresnelReflective;
            r -= refrAvg * fresnelRefractive;
            PTSS_DIAG_SCATTER(3, r < 0.0f);  // refraction lobe
            if (r < 0.0f) {
                // refrRay :516-531
                decided = true;
                if (sinT2 > 1.0f) ray.active = false;
                const float cosT = ptm::sqrt(1.0f - sinT2);
                const vec3 w_o = normalize(n * ray.d + (n * cosI - cosT) * normal);
                ray.o = point + (w_o * ptm::kRayBump);
                ray.d = w_o;
                result = v3(1, 1, 1);
            }
        }

        if (!decided) ray.active = false;  // absorbed, :316-317
    }

    PTSS_DIAG_SCATTER(4, kind != kLobeNone);       // the shared sampler tail
    PTSS_DIAG_SCATTER(5, kind == kLobeBeckmann);   // ... with the Beckmann elevation (atan, log) and the Cook-Torrance weight
    PTSS_DIAG_SCATTER(6, kind == kLobePhong);      // ... with the Phong elevation (pow)
    PTSS_DIAG_SCATTER(7, kind == kLobeLambert);
    if (kind != kLobeNone) {  // one copy of the sampler for every kind
        const float u1 = ptrng::uniform(ray.rng);
        const float u2 = ptrng::uniform(ray.rng);
        float azimuth, a, y;
        if (kind == kLobeBeckmann) {
            const float roughness = mat[3].w;
            const float theta = ptm::atan(-roughness * roughness * ptm::log(1.0f - u1));  // :564
            azimuth = u2 * 2 * ptm::kPi;                                                      // :565
            ptm::sincos(theta, a, y);  // m = (sinTheta * cosPhi, cosTheta, sinTheta * sinPhi), :567-569
        } else {
            azimuth = u1 * 2 * ptm::kPi;                                                      // :536, :550
            // :537-538, :551-552. u2 = k 2^-32 + 2^-33 rounded lies in [2^-33, 1], inside sqrt's fast range [2^-95, 2^96): no guard.
            // exponent + 1 of a lane that samples the Phong lobe (exponent != inf, above) is in rcp's range under kGuardPhongExponent.
            if (kind == kLobeLambert) y = ptm::sqrt_in_range(u2);
            else y = ptm::pow(u2, (guardFlags & kGuardPhongExponent) ? ptm::rcp_in_range(mMisc.x + 1) : ptm::rcp(mMisc.x + 1));
            a = ptm::sqrt(1 - y * y);                                                          // :539, :553
        }
        float sn, cs;
        ptm::sincos(azimuth, sn, cs);
        const vec3 sampled = rotate(rotateVectorToVector(v3(0, 1, 0), axis), v3(a * cs, y, a * sn));
        if (kind == kLobeBeckmann) {
            const vec3 beckmannNormal = sampled;
            // reflRay(ray, point, normal) :505-514
            const float cosB = ptm::abs(dot(ray.d, beckmannNormal));
            ray.d = ray.d - (2 * (-cosB)) * beckmannNormal;
            ray.o = point + (beckmannNormal * ptm::kRayBump);

            const vec3 half = normalize(ray.d - incident);
            const float nh = ptm::abs(dot(normal, half));
            const float nl = ptm::abs(dot(normal, ray.d));
            const float vh = ptm::abs(dot(incident, half));
            const float nv = ptm::abs(cosI);
            const float geometric = ptm::min(ptm::min(1.0f, ptm::div(2 * nh * nl, vh)), ptm::div(2 * nh * nv, vh));
            result = xyz(mSpecular) * geometric / nv;
        } else {
            ray.d = sampled;
        }
    }
    return result;
}

// one channel of writeToPixelsKernel, CudaTracer.cu:72-85: clamp, gamma 1/2.2, scale to 8 bits — in the proven-equal table
// form (ptquant.h): a hardware log2/exp2 guess settled by two exact threshold compares, ~12 instructions instead of the ~90
// of the software pow; three of these run for every wave that ends a path.
__device__ __forceinline__ uint32_t quantizeSample(float radiance, const float* T) { return ptq::quantize_fast(radiance, T); }

// The per-pixel home record of the random stream: 8 words (v0..v4, d, 2 pad) = one 32-byte sector, so
// parking or fetching a stream is two 16-byte accesses instead of six scattered 4-byte ones.
__device__ __forceinline__ void loadHome(const uint32_t* __restrict__ home, uint32_t p, ptrng::State& s) {
    const uint4 a = reinterpret_cast<const uint4*>(home)[2 * p];
    const uint4 b = reinterpret_cast<const uint4*>(home)[2 * p + 1];
    s.v[0] = a.x; s.v[1] = a.y; s.v[2] = a.z; s.v[3] = a.w;
    s.v[4] = b.x; s.d = b.y;
}
__device__ __forceinline__ void storeHome(uint32_t* __restrict__ home, uint32_t p, const ptrng::State& s) {
    reinterpret_cast<uint4*>(home)[2 * p] = uint4{s.v[0], s.v[1], s.v[2], s.v[3]};
    reinterpret_cast<uint4*>(home)[2 * p + 1] = uint4{s.v[4], s.d, 0u, 0u};
}

struct U3 {  // one totalPixelColors entry, moved as a single 12-byte access
    uint32_t x, y, z;
};

// A path ended: writeToPixelsKernel for this ray (CudaTracer.cu:63-104) + park the RNG stream.
// S == 1: the reference's read-modify-write of totalPixelColors and the display pixel, right here (one writer per pixel).
// S > 1: several lanes of a launch may end paths of the SAME pixel, so the tone-mapped 8-bit sample is parked in the
// stream's own word instead and displayKernel adds the S words of each pixel into the accumulator when the pass is
// complete (integer sums: order-free, still exact); the float sum is kept per stream (summed in lane order on read).
__device__ __forceinline__ void finishPath(const FrameBuffers& fb, const RayRegs& r, const float* quantT) {
    const uint32_t p = pixOf(r.pix), lane = laneOf(r.pix);
    const uint32_t stream = lane * fb.plane + p;
    const uint32_t qx = quantizeSample(r.L0.x, quantT), qy = quantizeSample(r.L0.y, quantT), qz = quantizeSample(r.L0.z, quantT);
    if (fb.samples == 1) {
        U3* acc = reinterpret_cast<U3*>(fb.accum) + p;
        U3 t = *acc;
        t.x += qx;
        t.y += qy;
        t.z += qz;
        *acc = t;
        if (fb.pixels) {
            const uint32_t px = (uint32_t)(unsigned char)(t.x * fb.inverseTicks + 0.5f) |
                                ((uint32_t)(unsigned char)(t.y * fb.inverseTicks + 0.5f) << 8) |
                                ((uint32_t)(unsigned char)(t.z * fb.inverseTicks + 0.5f) << 16) | (255u << 24);
            reinterpret_cast<uint32_t*>(fb.pixels)[p] = px;  // uchar4 {x, y, z, w = 255}
        }
    } else {
        // S > 1: every stream ends exactly one path per pass, so its 8-bit sample goes to the stream's own word with a
        // plain store; displayKernel adds the S words of a pixel into the accumulator at the end of the pass. (Three
        // atomics per path instead cost 34 % of the last-bounce kernel, where every ray finishes at once.)
        fb.staged[stream] = qx | (qy << 8) | (qz << 16);
    }
    if (fb.fsum) {
        float* fs = fb.fsum + 3u * stream;
        fs[0] += r.L0.x;
        fs[1] += r.L0.y;
        fs[2] += r.L0.z;
    }
    storeHome(fb.rngHome, stream, r.rng);
}

// ---- the loop guard with frame lanes (FrameBuffers, "frame lanes"): the frame's live count of bounce b >= 1 when this
// lane's own count `own` is not above the threshold. Waits (bounded) until every workgroup of each peer's bounce b - 1 has
// ended (the peer's done counters reach `target[p]`), then adds the peer's sixteen shard counters of bounce b.
// Called by at most one workgroup per shard of a lane that holds <= 128 rays, and by flushKernel.
// Every wait for a peer lane is bounded by TIME — about two seconds of the 100 MHz real-time counter (s_memrealtime), whatever
// a poll costs under load —: a peer stream that never runs must not hang the device. A wait that expires counts itself in
// guardTimeouts, which the host turns into PTSS_ETIMEOUT at its next synchronising call (ptss_api.hip checkLaneTimeouts).
constexpr unsigned long long kPeerWaitTicks = 200000000ull;
__device__ __forceinline__ bool peerWaitExpired(unsigned long long& since) {
    const unsigned long long now = wall_clock64();
    if (since == 0ull) {   // the first unsuccessful poll starts the clock
        since = now | 1ull;
        return false;
    }
    return now > since && now - since > kPeerWaitTicks;
}

__device__ __forceinline__ uint32_t frameLiveCount(const FrameBuffers& fb, int bounce, uint32_t own, const uint32_t* target) {
    uint32_t total = own;
    for (uint32_t p = 0; p < fb.numPeers; ++p) {
        unsigned long long since = 0ull;
        for (;;) {
            uint32_t ended = 0;
            for (int s = 0; s < kShards; ++s)
                ended += __hip_atomic_load(fb.peerDone[p] + countIndex(bounce - 1, s), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            // (>=, wrap-safe: lanes may run up to one frame apart, and a peer that is ahead has added its next frame's
            // workgroups already; its counts of THIS frame stay intact meanwhile — they live in the buffer its flushKernel
            // re-arms only after this lane's frame)
            if ((int32_t)(ended - target[p]) >= 0) break;
            __builtin_amdgcn_s_sleep(64);
            if (peerWaitExpired(since)) {
                if (threadIdx.x == 0) atomicAdd(fb.guardTimeouts, 1u);
                break;
            }
        }
        for (int s = 0; s < kShards; ++s)
            total += __hip_atomic_load(fb.peerCounts[p] + countIndex(bounce, s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return total;
}

}  // namespace
}  // namespace ptss
