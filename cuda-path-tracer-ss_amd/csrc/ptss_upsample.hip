// ptss_upsample.hip — the kernel behind ptss_upsample (include/ptss.h): a lo-res display image rebuilt at f times
// its size, guided by the features of both sizes. The arithmetic is csrc/ptupsample.h, shared with the host probe; this file only
// moves the data.
//
// One thread per HI-RES pixel, workgroups of 32 x 8 pixels (the denoiser's shape): a wave covers two hi-res rows of 32 pixels, i.e.
// two runs of 1 KiB of the hi-res features, and at factor f about 32 / f + 1 lo-res pixels per tap row: neighbouring lanes share
// their taps, which reach the L1 once per wave. Per pixel: both 16-byte rows of its own feature; for each of the four taps the
// material word, the 16-byte geometry row and the 4-byte colour; the nearest lo-res pixel's colour; the depth words of the four
// hi-res neighbours; one 4-byte pixel (and one 16-byte float entry, if asked for) is written. Every address is clamped into its
// frame (ptupsample.h), so all of these loads are unconditional and are issued before the first use of any of them: the wave waits
// once, not once per tap (the denoiser's waves spend 84 % of their cycles behind a load -> test -> load chain).
// Algorithmic traffic: 36 + 36 / f^2 bytes per hi-res pixel (+ 16 with the floats). No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "ptss_device.h"
#include "ptupsample.h"

namespace ptss {

constexpr int kUpsampleTileX = 32, kUpsampleTileY = 8;
static_assert(kUpsampleTileY == ptup::kTileRows, "ptss_upsample's row limit is stated for this tile");

// kFactor: the factor as a constant, so that the divisions and remainders of the tap geometry are multiplications and shifts
template <int kFactor>
__global__ __launch_bounds__(kUpsampleTileX* kUpsampleTileY) void upsampleKernel(const uint32_t* __restrict__ lo, const float4* __restrict__ featuresLo,
                                                                                 const float4* __restrict__ featuresHi, uint32_t* __restrict__ outHi,
                                                                                 float4* __restrict__ outFloat, int width, int height, ptdn::Level lv) {
    using namespace ptv;
    constexpr int factor = kFactor;
    const int X = blockIdx.x * kUpsampleTileX + (threadIdx.x % kUpsampleTileX);
    const int Y = blockIdx.y * kUpsampleTileY + (threadIdx.x / kUpsampleTileX);
    const int hiW = width * factor, hiH = height * factor;   // < 2^31 pixels together: ptss_upsample checks
    if (X >= hiW || Y >= hiH) return;   // every access below is to hi pixel (X, Y), or at coordinates upsamplePixel has clamped into a frame
    const size_t p = (size_t)Y * (size_t)hiW + (size_t)X;
    const float4 r0 = featuresHi[2 * p], r1 = featuresHi[2 * p + 1];
    const ptdn::Feature fp{v3(r0.x, r0.y, r0.z), r0.w, __builtin_bit_cast(int, r1.w)};
    auto colourAt = [&](int q) -> uint32_t { return lo[q]; };
    auto featureAt = [&](int q) -> ptdn::Feature {
        const float4 g = featuresLo[2 * (size_t)q];
        const int m = reinterpret_cast<const int*>(featuresLo)[8 * (size_t)q + 7];
        return ptdn::Feature{v3(g.x, g.y, g.z), g.w, m};
    };
    auto depthAt = [&](int x, int y) -> float { return reinterpret_cast<const float*>(featuresHi)[8 * ((size_t)y * (size_t)hiW + (size_t)x) + 3]; };
    const ptup::Result out = ptup::upsamplePixel(X, Y, width, height, factor, lv, fp, colourAt, featureAt, depthAt);
    outHi[p] = ptup::packBytes(out.colour);
    if (outFloat) outFloat[p] = float4{out.colour.x, out.colour.y, out.colour.z, out.weight};
}

hipError_t launchUpsample(hipStream_t st, const void* lo, const void* featuresLo, const void* featuresHi, void* outHi, void* outFloat, int width,
                          int height, int factor, const ptdn::Level& level, unsigned long long* launches) {
    const int hiW = width * factor, hiH = height * factor;
    const dim3 grid((unsigned)((hiW + kUpsampleTileX - 1) / kUpsampleTileX), (unsigned)((hiH + kUpsampleTileY - 1) / kUpsampleTileY));
    using Fn = void (*)(const uint32_t*, const float4*, const float4*, uint32_t*, float4*, int, int, ptdn::Level);
    static constexpr Fn table[ptup::kMaxFactor] = {upsampleKernel<1>, upsampleKernel<2>, upsampleKernel<3>, upsampleKernel<4>};
    if (factor < 1 || factor > ptup::kMaxFactor) return hipErrorInvalidValue;
    hipLaunchKernelGGL(table[factor - 1], grid, dim3(kUpsampleTileX * kUpsampleTileY), 0, st, static_cast<const uint32_t*>(lo),
                       static_cast<const float4*>(featuresLo), static_cast<const float4*>(featuresHi), static_cast<uint32_t*>(outHi),
                       static_cast<float4*>(outFloat), width, height, level);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++*launches;
    return e;
}

}  // namespace ptss
