// guards_device.hip — the helpers whose range guards are proven once against the guarded forms they replace and
// against the IEEE operations, on the device, bit for bit (signs of zero included; a NaN equals a NaN of any payload in the IEEE
// comparison only). Operands: every exponent x both signs x 64 mantissas (all-zero, all-one, one bit, random), +-0, infinities, NaNs,
// denormals, and the values within two ulps of every range end; vectors are made of three such values. Each set runs in two orders:
// sorted (waves hold neighbours: the wave-uniform tests pass or fail as a whole) and scattered (waves hold a mix: the escape with
// per-lane selects). Every check also counts the waves that took the unguarded path and those that did not: both must occur.
// Built by cuda-path-tracer-ss_amd/build.py (ptss_guardcheck), run by tests/test_gpu_guards.py. The cores' equality with IEEE
// inside their ranges is tests/csrc/math_exhaustive.hip's subject and is not repeated here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ptshade.h"

using namespace ptv;

namespace {

enum Check { kSqrtRcp = 0, kNormalize, kQuat, kUniformSum, kUniformSqrt, kLightSample, kLambertProven, kLambertGuarded, kRefraction, kExponent, kChecks };
const char* kNames[kChecks] = {"sqrt_rcp", "normalize_vec3", "normalize_quat", "rcp_uniform_sum", "sqrt_uniform", "light_sample",
                               "lambert_proven_powers", "lambert_guarded_powers", "refraction_index", "phong_exponent"};

struct Counts {
    unsigned long long checked, vsGuarded, vsIeee, fastWaves, escapedWaves;
};

__device__ bool sameBits(float a, float b) { return ptm::f2u(a) == ptm::f2u(b); }
__device__ bool sameValue(float a, float b) { return sameBits(a, b) || (a != a && b != b); }

__device__ void tally(Counts* c, bool badGuarded, bool badIeee, bool fastWave) {
    const unsigned long long active = __ballot(true);
    const unsigned long long g = __ballot(badGuarded), e = __ballot(badIeee);
    if (__lane_id() == (unsigned)(__ffsll((long long)active) - 1)) {
        atomicAdd(&c->checked, (unsigned long long)__popcll(active));
        atomicAdd(&c->vsGuarded, (unsigned long long)__popcll(g));
        atomicAdd(&c->vsIeee, (unsigned long long)__popcll(e));
        atomicAdd(fastWave ? &c->fastWaves : &c->escapedWaves, 1ull);
    }
}

// the forms before the change, written out
__device__ vec3 normalizeGuarded(vec3 v) { return v * ptm::rcp(ptm::sqrt(dot(v, v))); }
__device__ quat normalizeGuarded(quat q) {
    float len = ptm::sqrt(ptm::fma(q.w, q.w, ptm::fma(q.z, q.z, ptm::fma(q.y, q.y, q.x * q.x))));
    if (len <= 0.0f) return q4(1, 0, 0, 0);
    float inv = ptm::rcp(len);
    return q4(q.w * inv, q.x * inv, q.y * inv, q.z * inv);
}
__device__ float uniformOf(uint32_t x) { return (float)x * 2.3283064365386963e-10f + 1.1641532182693481e-10f; }   // ptrng::uniform's mapping

__device__ float pick(const float* v, uint32_t n, uint32_t i, uint32_t salt) {
    uint32_t h = (i + 1u) * 2654435761u ^ (salt * 0x9e3779b9u);
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    return v[h % n];
}

// one thread per operand (or per vector whose first component is operand i / reps); order: 0 sorted, 1 scattered
// sorted: the other components are the operand's neighbours in the list (same or adjacent exponent), so that a wave is of one kind
__global__ void checkKernel(int check, const float* v, uint32_t n, const float* aux, uint32_t nAux, uint32_t reps, int scattered, Counts* counts) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * reps) return;
    uint32_t i = t / reps;
    const uint32_t rep = t % reps;
    if (scattered) i = (uint32_t)(((unsigned long long)i * 40503ull + 12345ull * rep) % n);
    const float x = v[i];
    const float y = scattered ? pick(v, n, t, 1) : v[(i + 1u + rep) % n];
    const float z = scattered ? pick(v, n, t, 2) : v[(i + 2u + 3u * rep) % n];
    const float w = scattered ? pick(v, n, t, 3) : v[(i + 3u + 5u * rep) % n];
    const float other = scattered ? pick(aux, nAux, t, 4) : aux[(uint32_t)((unsigned long long)t * nAux / ((unsigned long long)n * reps))];
    Counts* c = counts + check;
    switch (check) {
    case kSqrtRcp: {
        float s, inv;
        ptm::sqrt_rcp(x, s, inv);
        const float gs = ptm::sqrt(x), gi = ptm::rcp(gs), is = __builtin_sqrtf(x), ii = 1.0f / is;
        tally(c, !sameBits(s, gs) || !sameBits(inv, gi), !sameValue(s, is) || !sameValue(inv, ii), ptm::every_lane(x >= ptm::kSqrtLo, x < ptm::kSqrtHi));
        break;
    }
    case kNormalize: {
        const vec3 a = v3(x, y, z), nw = normalize(a), g = normalizeGuarded(a);
        const float d = dot(a, a), ii = 1.0f / __builtin_sqrtf(d);
        const vec3 ie = a * ii;
        tally(c, !sameBits(nw.x, g.x) || !sameBits(nw.y, g.y) || !sameBits(nw.z, g.z),
              !sameValue(nw.x, ie.x) || !sameValue(nw.y, ie.y) || !sameValue(nw.z, ie.z), ptm::every_lane(d >= ptm::kSqrtLo, d < ptm::kSqrtHi));
        break;
    }
    case kQuat: {
        const quat a = q4(w, x, y, z), nw = normalize(a), g = normalizeGuarded(a);
        const float d = ptm::fma(a.w, a.w, ptm::fma(a.z, a.z, ptm::fma(a.y, a.y, a.x * a.x))), len = __builtin_sqrtf(d), ii = 1.0f / len;
        const quat ie = (len <= 0.0f) ? q4(1, 0, 0, 0) : q4(a.w * ii, a.x * ii, a.y * ii, a.z * ii);
        tally(c, !sameBits(nw.x, g.x) || !sameBits(nw.y, g.y) || !sameBits(nw.z, g.z) || !sameBits(nw.w, g.w),
              !sameValue(nw.x, ie.x) || !sameValue(nw.y, ie.y) || !sameValue(nw.z, ie.z) || !sameValue(nw.w, ie.w),
              ptm::every_lane(d >= ptm::kSqrtLo, d < ptm::kSqrtHi));
        break;
    }
    case kUniformSum: {   // the operands are draws: the bit patterns of the values, taken as 32-bit integers
        const float sum = uniformOf(ptm::f2u(x)) + uniformOf(ptm::f2u(y)) + uniformOf(ptm::f2u(z));
        const float nw = ptm::rcp_in_range(sum);
        tally(c, !sameBits(nw, ptm::rcp(sum)), !sameBits(nw, 1.0f / sum), true);
        break;
    }
    case kUniformSqrt: {
        const float u = uniformOf(ptm::f2u(x));
        const float nw = ptm::sqrt_in_range(u);
        tally(c, !sameBits(nw, ptm::sqrt(u)), !sameBits(nw, __builtin_sqrtf(u)), true);
        break;
    }
    case kLightSample: {
        const vec3 o = v3(x, y, z);
        float d2, dist;
        vec3 wi;
        ptss::lightSample(o, d2, dist, wi);
        const float gd2 = dot(o, o), gdist = ptm::sqrt(gd2);
        const vec3 gw = o / gdist;
        const float idist = __builtin_sqrtf(gd2);
        const vec3 iw = v3(o.x / idist, o.y / idist, o.z / idist);
        const float least = __builtin_fminf(__builtin_fminf(ptm::abs(o.x), ptm::abs(o.y)), ptm::abs(o.z));
        tally(c, !sameBits(d2, gd2) || !sameBits(dist, gdist) || !sameBits(wi.x, gw.x) || !sameBits(wi.y, gw.y) || !sameBits(wi.z, gw.z),
              !sameValue(dist, idist) || !sameValue(wi.x, iw.x) || !sameValue(wi.y, iw.y) || !sameValue(wi.z, iw.z),
              ptm::every_lane(ptm::in_light_window(gd2), least >= ptm::kDivLo));
        break;
    }
    case kLambertProven:     // powers: only values the scene classifier admits (the host filters them); distance2: anything
    case kLambertGuarded: {  // powers: anything, the scene's flag off
        const bool proven = check == kLambertProven;
        const float d2 = proven ? other : x;   // (proven: distance2 comes from the full list, whatever the admitted powers are)
        const vec3 power = proven ? v3(x, y, z) : v3(y, z, w);
        const float4 diffuse = float4{1.0f, 1.0f, 1.0f, 1.0f};
        vec3 nw = v3(0, 0, 0);
        ptss::addLambertTerm(nw, 1.0f, power, d2, diffuse, proven);
        const float divisor = (float)(4 * ptm::kPi * d2);
        const vec3 gl = power / divisor, il = v3(power.x / divisor, power.y / divisor, power.z / divisor);
        vec3 g = v3(0, 0, 0), ie = v3(0, 0, 0);
        g.x += 1.0f * gl.x * diffuse.x * diffuse.w * ptm::kInvPi; g.y += 1.0f * gl.y * diffuse.y * diffuse.w * ptm::kInvPi; g.z += 1.0f * gl.z * diffuse.z * diffuse.w * ptm::kInvPi;
        ie.x += 1.0f * il.x * diffuse.x * diffuse.w * ptm::kInvPi; ie.y += 1.0f * il.y * diffuse.y * diffuse.w * ptm::kInvPi; ie.z += 1.0f * il.z * diffuse.z * diffuse.w * ptm::kInvPi;
        tally(c, !sameBits(nw.x, g.x) || !sameBits(nw.y, g.y) || !sameBits(nw.z, g.z), !sameValue(nw.x, ie.x) || !sameValue(nw.y, ie.y) || !sameValue(nw.z, ie.z),
              proven && ptm::every_lane(ptm::in_light_window(d2)));
        break;
    }
    case kRefraction: {   // x: an index the classifier admits; both orientations of computeSinT2AndRefractiveIndexes
        const float a = ptm::div_in_range_operands(1.0f, x), b = ptm::div_in_range_operands(x, 1.0f);
        tally(c, !sameBits(a, ptm::div(1.0f, x)) || !sameBits(b, ptm::div(x, 1.0f)), !sameBits(a, 1.0f / x) || !sameBits(b, x / 1.0f), true);
        break;
    }
    case kExponent: {     // x: an exponent the classifier admits and the Phong sampler can meet (not +inf)
        const float nw = ptm::rcp_in_range(x + 1);
        tally(c, !sameBits(nw, ptm::rcp(x + 1)), !sameBits(nw, 1.0f / (x + 1)), true);
        break;
    }
    }
}

float u2f(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
uint32_t f2u(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

std::vector<float> structuredValues() {
    std::vector<uint32_t> mant = {0u, 1u, 0x7fffffu, 0x7ffffeu, 0x400000u};
    uint32_t s = 0x1234567u;
    while (mant.size() < 64) { s = s * 1664525u + 1013904223u; mant.push_back((s >> 9) & 0x7fffffu); }
    std::vector<float> v;
    for (uint32_t sign = 0; sign < 2; ++sign)
        for (uint32_t e = 0; e < 256; ++e)
            for (uint32_t m : mant) v.push_back(u2f((sign << 31) | (e << 23) | m));   // +-0, denormals, infinities and NaNs among them
    const float ends[] = {ptm::kSqrtLo, ptm::kSqrtHi, ptm::kRcpLo, ptm::kRcpHi, ptm::kDivLo, ptm::kDivHi, ptm::kLightD2Lo, ptm::kLightD2Hi,
                          0x1p-120f, 0x1p120f, 0x1p-47f, 0x1p48f};
    for (float e : ends)
        for (int d = -2; d <= 2; ++d)
            for (uint32_t sign = 0; sign < 2; ++sign) v.push_back(u2f((f2u(e) + (uint32_t)d) | (sign << 31)));
    return v;
}

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { printf("hip error %d at %s\n", (int)e_, #expr); return 2; } } while (0)

}  // namespace

int main() {
    const std::vector<float> all = structuredValues();
    std::vector<float> numerators, indices, exponents;
    for (float x : all) {
        if (ptm::fast_numerator(x)) numerators.push_back(x);
        if (ptm::fast_divisor(x)) indices.push_back(x);
        if (x != ptm::inf() && ptm::fast_rcp_operand(x + 1)) exponents.push_back(x);
    }
    numerators.push_back(0.0f);
    Counts* dCounts = nullptr;
    HIP_OK(hipMalloc(&dCounts, sizeof(Counts) * kChecks));
    HIP_OK(hipMemset(dCounts, 0, sizeof(Counts) * kChecks));
    float* dAll = nullptr;
    HIP_OK(hipMalloc(&dAll, all.size() * sizeof(float)));
    HIP_OK(hipMemcpy(dAll, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
    struct Run { int check; const std::vector<float>* values; uint32_t reps; };
    const Run runs[] = {{kSqrtRcp, &all, 1},       {kNormalize, &all, 24},       {kQuat, &all, 8},           {kUniformSum, &all, 8},
                        {kUniformSqrt, &all, 1},   {kLightSample, &all, 48},     {kLambertProven, &numerators, 24},
                        {kLambertGuarded, &all, 24}, {kRefraction, &indices, 1}, {kExponent, &exponents, 1}};
    for (const Run& r : runs) {
        const uint32_t n = (uint32_t)r.values->size();
        float* d = nullptr;
        HIP_OK(hipMalloc(&d, n * sizeof(float)));
        HIP_OK(hipMemcpy(d, r.values->data(), n * sizeof(float), hipMemcpyHostToDevice));
        const uint32_t threads = n * r.reps, blocks = (threads + 255u) / 256u;
        for (int scattered = 0; scattered < 2; ++scattered) {
            hipLaunchKernelGGL(checkKernel, dim3(blocks), dim3(256), 0, 0, r.check, d, n, dAll, (uint32_t)all.size(), r.reps, scattered, dCounts);
            HIP_OK(hipGetLastError());
        }
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(d));
    }
    Counts h[kChecks];
    HIP_OK(hipMemcpy(h, dCounts, sizeof(h), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(dCounts));
    HIP_OK(hipFree(dAll));
    unsigned long long bad = 0, total = 0;
    for (int k = 0; k < kChecks; ++k) {
        printf("%s checked=%llu vs_guarded=%llu vs_ieee=%llu fast_waves=%llu escaped_waves=%llu\n", kNames[k], h[k].checked, h[k].vsGuarded,
               h[k].vsIeee, h[k].fastWaves, h[k].escapedWaves);
        bad += h[k].vsGuarded + h[k].vsIeee;
        total += h[k].checked;
    }
    printf("total_checked=%llu total_mismatch=%llu\n", total, bad);
    return bad == 0 ? 0 : 1;
}
