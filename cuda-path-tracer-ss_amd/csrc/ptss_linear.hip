// ptss_linear.hip — the kernels behind ptss_accumulate_paths_linear and ptss_resolve_linear (include/ptss.h): a film that
// holds linear radiance as 64-bit fixed-point sums, order-free and exact for every index, and the resolve that turns it into linear means,
// display pixels and history entries (csrc/ptlinear.h has the arithmetic; its host build is the specification).
//
// With an index, the lanes of a wave that hold one pixel side by side are summed on chip first and the run's head lane alone issues the
// atomics (csrc/ptfilm.h sumRunsToHead, the reduction ptss_adaptive.hip uses).
#include "ptss_device.h"
#include "ptfilm.h"
#include "ptlinear.h"

namespace ptss {

using ptlin::u64;

constexpr int kLinearBlock = 256;

// a film entry as the two 16-byte rows it is read and written in: {r, g}, {b, samples | clamped << 32}
struct LinearRows {
    ulonglong2 rg, bc;
};

// without an index: ray i belongs to pixel firstPixel + i alone — a plain read-modify-write of the 32-byte entry
__global__ __launch_bounds__(kLinearBlock) void linearAccumulateKernel(const float4* __restrict__ results, uint32_t firstPixel, uint32_t n,
                                                                       ulonglong2* __restrict__ film, ptlin::Scale sc) {
    const uint32_t i = blockIdx.x * kLinearBlock + threadIdx.x;
    if (i >= n) return;
    const float4 r = results[i];
    u64 q[3];
    const uint32_t flag = ptlin::sampleToFixed(r.x, r.y, r.z, sc, q);
    ulonglong2* e = film + 2 * (size_t)(firstPixel + i);
    ulonglong2 rg = e[0], bc = e[1];
    rg.x += q[0];
    rg.y += q[1];
    bc.x += q[2];
    bc.y += 1ull | ((u64)flag << 32);   // samples and clamped, each in its own half while samples < 2^32
    e[0] = rg;
    e[1] = bc;
}

// with an index: the runs of equal, in-range pixels inside a wave are summed by a segmented reduction towards the run's first lane,
// which alone issues the four 64-bit atomics. A run is split at the wave's edge, and duplicates that are not neighbours meet in the
// atomics, so the sums are exact for every index. A sample is at most 2^40 and a wave's run at most 64 * 2^40 = 2^46: a channel travels as
// two 32-bit words; the counts, at most 64 each, share one (samples | clamped << 16). Seven words travel, six steps each.
__global__ __launch_bounds__(kLinearBlock) void linearScatterKernel(const float4* __restrict__ results, const uint32_t* __restrict__ index, uint32_t n,
                                                                    u64* __restrict__ film, uint32_t filmPixels, ptlin::Scale sc,
                                                                    unsigned long long* __restrict__ rejected) {
    const uint32_t i = blockIdx.x * kLinearBlock + threadIdx.x;
    const bool inBatch = i < n;
    const uint32_t p = inBatch ? index[i] : 0u;
    const bool ok = inBatch && p < filmPixels;
    countDropped(inBatch && !ok, rejected);
    const uint32_t key = ok ? p : 0xffffffffu;   // (a film has fewer than 2^31 pixels) lanes without a pixel carry zeros and never lead a store
    u64 q[3] = {0ull, 0ull, 0ull};
    uint32_t counts = 0u;
    if (ok) {
        const float4 r = results[i];
        counts = 1u | (ptlin::sampleToFixed(r.x, r.y, r.z, sc, q) << 16);
    }
    const bool head = sumRunsToHead(key, [&](uint32_t d, bool joins) {
        const u64 r2 = (u64)__shfl_down((long long)q[0], d, 64), g2 = (u64)__shfl_down((long long)q[1], d, 64),
                  b2 = (u64)__shfl_down((long long)q[2], d, 64);
        const uint32_t c2 = (uint32_t)__shfl_down((int)counts, d, 64);
        if (joins) {
            q[0] += r2;
            q[1] += g2;
            q[2] += b2;
            counts += c2;
        }
    });
    if (!(head && ok)) return;
    u64* e = film + 4 * (size_t)p;
    atomicAdd(e + 0, q[0]);
    atomicAdd(e + 1, q[1]);
    atomicAdd(e + 2, q[2]);
    atomicAdd(e + 3, (u64)(counts & 0xffffu) | ((u64)(counts >> 16) << 32));   // samples | clamped << 32, one word
}

// one streaming pass over pixels firstPixel .. firstPixel + count; each output may be null
__global__ __launch_bounds__(kLinearBlock) void linearResolveKernel(const ulonglong2* __restrict__ film, uint32_t firstPixel, uint32_t count,
                                                                    ptlin::Scale sc, const float* __restrict__ quantT, float4* __restrict__ linear,
                                                                    ptss_uchar4* __restrict__ pixels, float4* __restrict__ history) {
    const uint32_t i = blockIdx.x * kLinearBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t p = firstPixel + i;
    const ulonglong2 rg = film[2 * (size_t)p], bc = film[2 * (size_t)p + 1];
    float lin[4], hist[4];
    uint32_t px;
    ptlin::resolve(rg.x, rg.y, bc.x, (uint32_t)bc.y, sc, quantT, lin, &px, hist);
    if (linear) linear[p] = float4{lin[0], lin[1], lin[2], lin[3]};
    if (pixels) reinterpret_cast<uint32_t*>(pixels)[p] = px;   // uchar4 {x, y, z, w = 255}
    if (history) history[p] = float4{hist[0], hist[1], hist[2], hist[3]};
}

hipError_t launchLinearAccumulate(hipStream_t st, const void* results, const uint32_t* index, uint32_t firstPixel, uint32_t n, void* film,
                                  uint32_t filmPixels, const ptss_linear_params& params, unsigned long long* rejected,
                                  unsigned long long* launches) {
    const dim3 grid(filmBlocksFor(n, kLinearBlock)), block(kLinearBlock);
    const ptlin::Scale sc = ptlin::scaleOf(params);
    if (!index)
        hipLaunchKernelGGL(linearAccumulateKernel, grid, block, 0, st, static_cast<const float4*>(results), firstPixel, n,
                           static_cast<ulonglong2*>(film), sc);
    else
        hipLaunchKernelGGL(linearScatterKernel, grid, block, 0, st, static_cast<const float4*>(results), index, n, static_cast<u64*>(film),
                           filmPixels, sc, rejected);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++*launches;
    return e;
}

hipError_t launchLinearResolve(hipStream_t st, const void* film, uint32_t firstPixel, uint32_t count, const ptss_linear_params& params,
                               const float* quantTable, void* linear, ptss_uchar4* pixels, void* history, unsigned long long* launches) {
    hipLaunchKernelGGL(linearResolveKernel, dim3(filmBlocksFor(count, kLinearBlock)), dim3(kLinearBlock), 0, st, static_cast<const ulonglong2*>(film),
                       firstPixel, count, ptlin::scaleOf(params), quantTable, static_cast<float4*>(linear), pixels, static_cast<float4*>(history));
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++*launches;
    return e;
}

}  // namespace ptss
