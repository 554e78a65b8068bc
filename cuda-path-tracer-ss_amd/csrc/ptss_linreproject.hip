// ptss_linreproject.hip — the kernel behind ptss_reproject_linear (include/ptss.h): the previous pose's linear film
// seeds the new pose's film and moments. The arithmetic is csrc/ptlinrp.h, shared with the host probe (ptss_probe_reproject_linear,
// the specification); this file only moves the data.
//
// One thread per pixel of the new film, workgroups of 32 x 8 pixels laid out as one row of workgroups (a film 2^22 pixels high has more
// tile rows than a grid has in y); the tile's coordinates come from the workgroup index on the scalar unit. Both cameras travel by
// value. Per pixel one feature (two 16-byte rows; with kMotion one more 16-byte row), then up to four taps of the previous pose, in
// reprojectKernel's order: the material word first, the 16-byte geometry row behind a match, the 32-byte film entry behind that and
// the 32-byte moment row behind a non-empty entry; the 64-bit divisions and ptls::standardError run only for taps that count. One
// 32-byte film row and (kMoments) one 32-byte moment row are written per pixel, empty pixels included: the call writes all of both.
// The four counters of ptss_reproject_linear_info: a wave's ballots are counted on the scalar unit, lane 0 of each wave adds them to
// four LDS words (16 B, the kernel's only LDS; one barrier), and threads 0 .. 3 add the non-zero ones to the caller's with one
// 64-bit vector atomic each: integer adds, the same bytes for every launch shape. No workgroup waits for another.
#include <hip/hip_runtime.h>

#include "ptlinrp.h"
#include "ptss_device.h"

namespace ptss {

using ptlin::u64;

constexpr int kLinReprojectTileX = 32, kLinReprojectTileY = 8;
constexpr int kLinReprojectBlock = kLinReprojectTileX * kLinReprojectTileY;

template <bool kSplat, bool kMoments, bool kMotion>
__global__ __launch_bounds__(kLinReprojectBlock) void linReprojectKernel(const float4* __restrict__ featuresNow, const float4* __restrict__ motionNow,
                                                                         const float4* __restrict__ featuresPrev,
                                                                         const ulonglong2* __restrict__ filmPrev,
                                                                         const ulonglong2* __restrict__ momentsPrev, ulonglong2* __restrict__ filmOut,
                                                                         ulonglong2* __restrict__ momentsOut, unsigned long long* __restrict__ info,
                                                                         int tilesX, ptcam::Film now, ptlrp::Prev prev, ptlrp::Rule R) {
    using namespace ptv;
    __shared__ uint32_t sCount[4];
    const int tileX = (int)(blockIdx.x % (unsigned)tilesX), tileY = (int)(blockIdx.x / (unsigned)tilesX);
    const int x = tileX * kLinReprojectTileX + (int)(threadIdx.x % kLinReprojectTileX);
    const int y = tileY * kLinReprojectTileY + (int)(threadIdx.x / kLinReprojectTileX);
    const bool inside = x < now.width && y < now.height;   // every access below is to pixel (x, y) or to a tap seedPixel has bounds-checked
    if (info && threadIdx.x < 4) sCount[threadIdx.x] = 0u;
    int status = -1;
    bool noVariance = false;
    if (inside) {
        const size_t p = (size_t)y * (size_t)now.width + (size_t)x;
        const float4 r0 = featuresNow[2 * p];
        const ptdn::Feature fp{v3(r0.x, r0.y, r0.z), r0.w, reinterpret_cast<const int*>(featuresNow)[8 * p + 7]};
        auto pointOf = [&](vec3 o, vec3 d) -> vec3 {
            if constexpr (kMotion) {
                const float4 m = motionNow[p];
                return v3(m.x, m.y, m.z);
            } else {
                return madd(d, fp.depth, o);
            }
        };
        auto materialAt = [&](size_t q) -> int { return reinterpret_cast<const int*>(featuresPrev)[8 * q + 7]; };
        auto geometryAt = [&](size_t q) -> ptrp::Geometry {
            const float4 g = featuresPrev[2 * q];
            return ptrp::Geometry{v3(g.x, g.y, g.z), g.w};
        };
        auto entryAt = [&](size_t q, u64* e) {
            const ulonglong2 rg = filmPrev[2 * q], bw = filmPrev[2 * q + 1];
            e[0] = rg.x, e[1] = rg.y, e[2] = bw.x, e[3] = bw.y;
        };
        auto momentAt = [&](size_t q, u64* m) {
            const ulonglong2 a = momentsPrev[2 * q], b = momentsPrev[2 * q + 1];
            m[0] = a.x, m[1] = a.y, m[2] = b.x, m[3] = b.y;
        };
        ptlrp::Seed s;
        ptlrp::seedPixel<kMoments>(x, y, fp, now, prev, R, kSplat, pointOf, materialAt, geometryAt, entryAt, momentAt, s);
        filmOut[2 * p] = ulonglong2{s.film[0], s.film[1]};
        filmOut[2 * p + 1] = ulonglong2{s.film[2], s.film[3]};
        if constexpr (kMoments) {
            momentsOut[2 * p] = ulonglong2{s.moment[0], s.moment[1]};
            momentsOut[2 * p + 1] = ulonglong2{s.moment[2], s.moment[3]};
        }
        status = s.status;
        noVariance = s.noVariance;
    }
    if (info) {   // wave-uniform: a kernel argument
        __syncthreads();
        const uint32_t seeded = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(status == ptlrp::kSeeded));
        const uint32_t offFilm = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(status == ptlrp::kOffFilm));
        const uint32_t noTap = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(status == ptlrp::kNoTap));
        const uint32_t noVar = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(noVariance));
        if ((threadIdx.x & 63u) == 0u) {
            if (seeded) atomicAdd(&sCount[0], seeded);
            if (offFilm) atomicAdd(&sCount[1], offFilm);
            if (noTap) atomicAdd(&sCount[2], noTap);
            if (noVar) atomicAdd(&sCount[3], noVar);
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const uint32_t c = sCount[threadIdx.x];
            if (c) atomicAdd(&info[threadIdx.x], (unsigned long long)c);
        }
    }
}

using LinReprojectFn = void (*)(const float4*, const float4*, const float4*, const ulonglong2*, const ulonglong2*, ulonglong2*, ulonglong2*,
                                unsigned long long*, int, ptcam::Film, ptlrp::Prev, ptlrp::Rule);

template <bool kSplat, bool kMoments>
static LinReprojectFn linReprojectOf(bool motion) {
    return motion ? linReprojectKernel<kSplat, kMoments, true> : linReprojectKernel<kSplat, kMoments, false>;
}

hipError_t launchLinearReproject(hipStream_t st, const ptss_film_camera& now, const void* featuresNow, const void* motionNow,
                                 const ptss_film_camera& prev, const void* featuresPrev, const void* filmPrev, bool splat, const void* momentsPrev,
                                 const ptss_linear_params& film, const ptss_reproject_linear_params& params, void* filmOut, void* momentsOut,
                                 void* info, unsigned long long* launches) {
    const bool moments = momentsPrev != nullptr, motion = motionNow != nullptr;
    const LinReprojectFn fn = splat ? (moments ? linReprojectOf<true, true>(motion) : linReprojectOf<true, false>(motion))
                                    : (moments ? linReprojectOf<false, true>(motion) : linReprojectOf<false, false>(motion));
    // the tiles of the film as one row of workgroups; below 2^31 / 8 + 2^22
    const int tilesX = (now.width + kLinReprojectTileX - 1) / kLinReprojectTileX, tilesY = (now.height + kLinReprojectTileY - 1) / kLinReprojectTileY;
    const dim3 grid((unsigned)tilesX * (unsigned)tilesY);
    hipLaunchKernelGGL(fn, grid, dim3(kLinReprojectBlock), 0, st, static_cast<const float4*>(featuresNow), static_cast<const float4*>(motionNow),
                       static_cast<const float4*>(featuresPrev), static_cast<const ulonglong2*>(filmPrev), static_cast<const ulonglong2*>(momentsPrev),
                       static_cast<ulonglong2*>(filmOut), static_cast<ulonglong2*>(momentsOut), static_cast<unsigned long long*>(info), tilesX,
                       ptlrp::nowOf(now), ptlrp::prevOf(prev), ptlrp::ruleOf(params, film));
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++*launches;
    return e;
}

}  // namespace ptss
