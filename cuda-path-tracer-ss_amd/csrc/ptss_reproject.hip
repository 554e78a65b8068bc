// ptss_reproject.hip — the kernel behind ptss_reproject (include/ptss.h): the history of the previous camera pose
// carried into the current frame. The arithmetic is csrc/ptreproject.h, shared with the host probe; this file only moves the data.
//
// One thread per pixel, workgroups of 32 x 8 pixels (the denoiser's shape): a wave covers two rows of 32 pixels. Per pixel one
// feature (two 16-byte rows) and one accumulator entry (12 B) are read, then up to four taps of the previous frame: the material
// word first, the geometry row and the 16-byte history entry only behind a matching material; one 16-byte entry is written.
// Neighbouring pixels reproject to neighbouring taps, so a wave's loads of one tap are two runs of about 32 entries except at
// silhouettes; the four taps of a pixel share their cache lines through the L1 / L2. No LDS, no scratch.
// historyPrev = nullptr: "no history", every pixel gets (c, n).
// reprojectKernel<true> is ptss_reproject_motion: the same body with the point of a hit read from a motion row.
#include <hip/hip_runtime.h>

#include "ptreproject.h"
#include "ptss_device.h"

namespace ptss {

constexpr int kReprojectTileX = 32, kReprojectTileY = 8;

// kMotion (ptss_reproject_motion): a hit pixel's point comes from its ptss_pixel_motion row, one more 16-byte load
// per pixel. Without kMotion the argument is empty.
template <bool kMotion>
struct ReprojectMotion {};
template <>
struct ReprojectMotion<true> {
    const float4* now;
};

template <bool kMotion>
__global__ __launch_bounds__(kReprojectTileX* kReprojectTileY) void reprojectKernel(
    const uint32_t* __restrict__ accum, const float4* __restrict__ featuresNow, const float4* __restrict__ featuresPrev,
    const float4* __restrict__ historyPrev, float4* __restrict__ historyOut, int width, int height, ptrp::View now, ptrp::View prev,
    ptrp::Params prm, float inverseTicks, float n, ReprojectMotion<kMotion> motion) {
    using namespace ptv;
    const int x = blockIdx.x * kReprojectTileX + (threadIdx.x % kReprojectTileX);
    const int y = blockIdx.y * kReprojectTileY + (threadIdx.x / kReprojectTileX);
    if (x >= width || y >= height) return;   // every access below is to pixel (x, y) or to a tap reprojectPixel has bounds-checked
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const uint32_t* a = accum + 3 * p;
    const vec3 cp = ptdn::displayValue(a[0], a[1], a[2], inverseTicks);
    ptrp::Entry out{cp, n};
    if (historyPrev) {
        const float4 r0 = featuresNow[2 * p];
        const ptdn::Feature fp{v3(r0.x, r0.y, r0.z), r0.w, reinterpret_cast<const int*>(featuresNow)[8 * p + 7]};
        auto materialAt = [&](int q) -> int { return reinterpret_cast<const int*>(featuresPrev)[8 * (size_t)q + 7]; };
        auto geometryAt = [&](int q) -> ptrp::Geometry {
            const float4 g = featuresPrev[2 * (size_t)q];
            return ptrp::Geometry{v3(g.x, g.y, g.z), g.w};
        };
        auto historyAt = [&](int q) -> ptrp::Entry {
            const float4 h = historyPrev[q];
            return ptrp::Entry{v3(h.x, h.y, h.z), h.w};
        };
        if constexpr (kMotion) {
            const float4 m = motion.now[p];
            auto pointOf = [&](vec3) -> vec3 { return v3(m.x, m.y, m.z); };
            out = ptrp::reprojectPixel(x, y, width, height, cp, n, fp, now, prev, prm, pointOf, materialAt, geometryAt, historyAt);
        } else {
            out = ptrp::reprojectPixel(x, y, width, height, cp, n, fp, now, prev, prm, materialAt, geometryAt, historyAt);
        }
    }
    historyOut[p] = float4{out.colour.x, out.colour.y, out.colour.z, out.weight};
}

template <bool kMotion>
static hipError_t launchReprojectKernel(hipStream_t st, const uint32_t* accum, const void* featuresNow, ReprojectMotion<kMotion> motion,
                                        const void* featuresPrev, const void* historyPrev, void* historyOut, int width, int height,
                                        const ptrp::View& now, const ptrp::View& prev, const ptrp::Params& params, float inverseTicks, float n,
                                        unsigned long long* launched) {
    const dim3 grid((unsigned)((width + kReprojectTileX - 1) / kReprojectTileX), (unsigned)((height + kReprojectTileY - 1) / kReprojectTileY));
    hipLaunchKernelGGL(reprojectKernel<kMotion>, grid, dim3(kReprojectTileX * kReprojectTileY), 0, st, accum, static_cast<const float4*>(featuresNow),
                       static_cast<const float4*>(featuresPrev), static_cast<const float4*>(historyPrev), static_cast<float4*>(historyOut),
                       width, height, now, prev, params, inverseTicks, n, motion);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) markLaunched(launched, kMotion ? PTSS_KERNEL_REPROJECT_MOTION : PTSS_KERNEL_REPROJECT);
    return e;
}

hipError_t launchReproject(hipStream_t st, const uint32_t* accum, const void* featuresNow, const void* featuresPrev, const void* historyPrev,
                           void* historyOut, int width, int height, const ptrp::View& now, const ptrp::View& prev, const ptrp::Params& params,
                           float inverseTicks, float n, unsigned long long* launched) {
    return launchReprojectKernel(st, accum, featuresNow, ReprojectMotion<false>{}, featuresPrev, historyPrev, historyOut, width, height, now, prev,
                                 params, inverseTicks, n, launched);
}

hipError_t launchReprojectMotion(hipStream_t st, const uint32_t* accum, const void* featuresNow, const void* motionNow, const void* featuresPrev,
                                 const void* historyPrev, void* historyOut, int width, int height, const ptrp::View& now, const ptrp::View& prev,
                                 const ptrp::Params& params, float inverseTicks, float n, unsigned long long* launched) {
    return launchReprojectKernel(st, accum, featuresNow, ReprojectMotion<true>{static_cast<const float4*>(motionNow)}, featuresPrev, historyPrev,
                                 historyOut, width, height, now, prev, params, inverseTicks, n, launched);
}

}  // namespace ptss
