// ptss_denoise.hip — the kernel behind ptss_denoise (include/ptss.h): one pass of the edge-avoiding A-trous
// filter per launch. The arithmetic is csrc/ptdenoise.h, shared with the host probe; this file only moves the data.
//
// One thread per pixel, workgroups of 32 x 8 pixels: a wave covers two rows of 32 pixels, so a tap row is two 512-byte runs of
// 16-byte colour loads and two 1-KiB runs of features. Every tap is read from global memory at every spacing: at 1080p the colour
// plane is 33 MB and the features 66 MB, which the Infinity Cache holds between passes; neighbouring pixels share their taps
// through the L1 / L2 at spacings 1 and 2 and through the L2 / Infinity Cache beyond. (Staging the tile plus halo in LDS at
// spacings 1 and 2 has not been built or measured. Measured for this plain form, DESIGN.md §3.17: every level costs the same, the
// vector ALU is busy 60 % of a pass or more, and the waves wait on the dependent material -> colour -> feature-row loads of a tap
// for 84 % of their resident cycles — staging, or issuing the material loads ahead of the loop, is what would attack that.)
// kFirst: the pass reads the integer accumulator and converts it on the fly; kLast: it writes the display bytes — there are no
// separate conversion kernels. levels = 0 is the pass <true, true> with radius 0.
#include <hip/hip_runtime.h>

#include "ptdenoise.h"
#include "ptss_device.h"

namespace ptss {

constexpr int kDenoiseTileX = 32, kDenoiseTileY = 8;

template <bool kFirst, bool kLast>
__global__ __launch_bounds__(kDenoiseTileX* kDenoiseTileY) void denoiseKernel(const void* __restrict__ src, void* __restrict__ dst,
                                                                              const float4* __restrict__ features, int width, int height,
                                                                              ptdn::Level lv, float inverseTicks) {
    using namespace ptv;
    const int x = blockIdx.x * kDenoiseTileX + (threadIdx.x % kDenoiseTileX);
    const int y = blockIdx.y * kDenoiseTileY + (threadIdx.x / kDenoiseTileX);
    if (x >= width || y >= height) return;   // every access below is to pixel (x, y) or to a tap filterPixel has bounds-checked
    auto colourAt = [&](int q) -> vec3 {
        if constexpr (kFirst) {
            const uint32_t* a = static_cast<const uint32_t*>(src) + 3 * (size_t)q;
            return ptdn::displayValue(a[0], a[1], a[2], inverseTicks);
        } else {
            const float4 c = static_cast<const float4*>(src)[q];
            return v3(c.x, c.y, c.z);
        }
    };
    auto featureAt = [&](int q) -> ptdn::Feature {
        const float4 r0 = features[2 * (size_t)q];
        const int m = reinterpret_cast<const int*>(features)[8 * (size_t)q + 7];
        return ptdn::Feature{v3(r0.x, r0.y, r0.z), r0.w, m};
    };
    auto depthAt = [&](int q) -> float { return reinterpret_cast<const float*>(features)[8 * (size_t)q + 3]; };
    const vec3 out = ptdn::filterPixel(x, y, width, height, lv, colourAt, featureAt, depthAt);
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    if constexpr (kLast) {
        const uint32_t px = (uint32_t)ptdn::toByte(out.x) | ((uint32_t)ptdn::toByte(out.y) << 8) | ((uint32_t)ptdn::toByte(out.z) << 16) | (255u << 24);
        static_cast<uint32_t*>(dst)[p] = px;   // uchar4 {x, y, z, w = 255}
    } else {
        static_cast<float4*>(dst)[p] = float4{out.x, out.y, out.z, 0.0f};
    }
}

hipError_t launchDenoise(hipStream_t st, bool first, bool last, const void* src, void* dst, const void* features, int width, int height,
                         const ptdn::Level& level, float inverseTicks, unsigned long long* launched) {
    using Fn = void (*)(const void*, void*, const float4*, int, int, ptdn::Level, float);
    static constexpr Fn table[4] = {denoiseKernel<false, false>, denoiseKernel<false, true>, denoiseKernel<true, false>, denoiseKernel<true, true>};
    const dim3 grid((unsigned)((width + kDenoiseTileX - 1) / kDenoiseTileX), (unsigned)((height + kDenoiseTileY - 1) / kDenoiseTileY));
    hipLaunchKernelGGL(table[(first ? 2 : 0) + (last ? 1 : 0)], grid, dim3(kDenoiseTileX * kDenoiseTileY), 0, st, src, dst,
                       static_cast<const float4*>(features), width, height, level, inverseTicks);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) markLaunched(launched, PTSS_KERNEL_DENOISE);
    return e;
}

}  // namespace ptss
