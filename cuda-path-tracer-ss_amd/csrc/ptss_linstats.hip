// ptss_linstats.hip — the accumulate kernels behind ptss_accumulate_paths_linear_stats (include/ptss.h): a linear film
// that also keeps the luminance moments of its fixed-point samples (csrc/ptlinstats.h has the arithmetic; its host build is the
// specification). The film's bytes are those of ptss_linear.hip's kernels — the same ptlin::sampleToFixed, the same words — and the film
// may be absent: a filtered film keeps its moments by home pixel beside ptss_splat_paths. The plan that reads the moments
// (ptss_plan_samples_linear) lives beside the scan it shares, in ptss_adaptive.hip.
//
// With an index, the lanes of a wave that hold one pixel side by side are summed on chip first and the run's head lane alone issues the
// atomics (csrc/ptfilm.h sumRunsToHead, the reduction ptss_adaptive.hip and ptss_linear.hip use).
#include "ptss_device.h"
#include "ptfilm.h"
#include "ptlinstats.h"

namespace ptss {

using ptlin::u64;

constexpr int kLinStatsBlock = 256;

// without an index: ray i belongs to pixel firstPixel + i alone — a plain read-modify-write of the 32-byte moment row and, with a film,
// of the 32-byte entry (linearAccumulateKernel's bytes)
template <bool kFilm>
__global__ __launch_bounds__(kLinStatsBlock) void linStatsAccumulateKernel(const float4* __restrict__ results, uint32_t firstPixel, uint32_t n,
                                                                           ulonglong2* __restrict__ film, ulonglong2* __restrict__ moments,
                                                                           ptlin::Scale sc) {
    const uint32_t i = blockIdx.x * kLinStatsBlock + threadIdx.x;
    if (i >= n) return;
    const float4 r = results[i];
    u64 q[3];
    const uint32_t flag = ptlin::sampleToFixed(r.x, r.y, r.z, sc, q);
    const ptls::Sample s = ptls::sampleOf(q[0], q[1], q[2]);
    const size_t p = (size_t)firstPixel + i;
    ulonglong2* m = moments + 2 * p;
    ulonglong2 ys = m[0], hn = m[1];
    ys.x += s.y;
    ys.y += s.lo;
    hn.x += s.hi;
    hn.y += 1ull;
    m[0] = ys;
    m[1] = hn;
    if (kFilm) {
        ulonglong2* e = film + 2 * p;
        ulonglong2 rg = e[0], bc = e[1];
        rg.x += q[0];
        rg.y += q[1];
        bc.x += q[2];
        bc.y += 1ull | ((u64)flag << 32);   // samples and clamped, each in its own half while samples < 2^32
        e[0] = rg;
        e[1] = bc;
    }
}

// with an index: linearScatterKernel's reduction with the moment's words beside the film's. A sample's y, lo and hi are at most 2^40 and a
// wave's run at most 64 * 2^40 = 2^46: each travels as two 32-bit words, like a channel; the counts, at most 64 each, share one
// (samples | clamped << 16). Seven words travel without a film, thirteen with one, six steps each. Only a run's head issues atomics: four
// 64-bit adds for the moment row, four more for the film.
template <bool kFilm>
__global__ __launch_bounds__(kLinStatsBlock) void linStatsScatterKernel(const float4* __restrict__ results, const uint32_t* __restrict__ index,
                                                                        uint32_t n, u64* __restrict__ film, u64* __restrict__ moments,
                                                                        uint32_t filmPixels, ptlin::Scale sc,
                                                                        unsigned long long* __restrict__ rejected) {
    const uint32_t i = blockIdx.x * kLinStatsBlock + threadIdx.x;
    const bool inBatch = i < n;
    const uint32_t p = inBatch ? index[i] : 0u;
    const bool ok = inBatch && p < filmPixels;
    countDropped(inBatch && !ok, rejected);
    const uint32_t key = ok ? p : 0xffffffffu;   // (a film has fewer than 2^31 pixels) lanes without a pixel carry zeros and never lead a store
    u64 q[3] = {0ull, 0ull, 0ull};
    ptls::Sample s{0ull, 0ull, 0ull};
    uint32_t counts = 0u;
    if (ok) {
        const float4 r = results[i];
        counts = 1u | (ptlin::sampleToFixed(r.x, r.y, r.z, sc, q) << 16);
        s = ptls::sampleOf(q[0], q[1], q[2]);
    }
    const bool head = sumRunsToHead(key, [&](uint32_t d, bool joins) {
        const u64 y2 = (u64)__shfl_down((long long)s.y, d, 64), lo2 = (u64)__shfl_down((long long)s.lo, d, 64),
                  hi2 = (u64)__shfl_down((long long)s.hi, d, 64);
        const uint32_t c2 = (uint32_t)__shfl_down((int)counts, d, 64);
        u64 r2 = 0ull, g2 = 0ull, b2 = 0ull;
        if (kFilm) {
            r2 = (u64)__shfl_down((long long)q[0], d, 64);
            g2 = (u64)__shfl_down((long long)q[1], d, 64);
            b2 = (u64)__shfl_down((long long)q[2], d, 64);
        }
        if (joins) {
            s.y += y2;
            s.lo += lo2;
            s.hi += hi2;
            counts += c2;
            if (kFilm) {
                q[0] += r2;
                q[1] += g2;
                q[2] += b2;
            }
        }
    });
    if (!(head && ok)) return;
    u64* m = moments + 4 * (size_t)p;
    atomicAdd(m + 0, s.y);
    atomicAdd(m + 1, s.lo);
    atomicAdd(m + 2, s.hi);
    atomicAdd(m + 3, (u64)(counts & 0xffffu));
    if (kFilm) {
        u64* e = film + 4 * (size_t)p;
        atomicAdd(e + 0, q[0]);
        atomicAdd(e + 1, q[1]);
        atomicAdd(e + 2, q[2]);
        atomicAdd(e + 3, (u64)(counts & 0xffffu) | ((u64)(counts >> 16) << 32));   // samples | clamped << 32, one word
    }
}

hipError_t launchLinStatsAccumulate(hipStream_t st, const void* results, const uint32_t* index, uint32_t firstPixel, uint32_t n, void* film,
                                    void* moments, uint32_t filmPixels, const ptss_linear_params& params, unsigned long long* rejected,
                                    unsigned long long* launches) {
    const dim3 grid(filmBlocksFor(n, kLinStatsBlock)), block(kLinStatsBlock);
    const ptlin::Scale sc = ptlin::scaleOf(params);
    const float4* res = static_cast<const float4*>(results);
    if (!index) {
        ulonglong2* f = static_cast<ulonglong2*>(film);
        ulonglong2* m = static_cast<ulonglong2*>(moments);
        if (film)
            hipLaunchKernelGGL(linStatsAccumulateKernel<true>, grid, block, 0, st, res, firstPixel, n, f, m, sc);
        else
            hipLaunchKernelGGL(linStatsAccumulateKernel<false>, grid, block, 0, st, res, firstPixel, n, f, m, sc);
    } else {
        u64* f = static_cast<u64*>(film);
        u64* m = static_cast<u64*>(moments);
        if (film)
            hipLaunchKernelGGL(linStatsScatterKernel<true>, grid, block, 0, st, res, index, n, f, m, filmPixels, sc, rejected);
        else
            hipLaunchKernelGGL(linStatsScatterKernel<false>, grid, block, 0, st, res, index, n, f, m, filmPixels, sc, rejected);
    }
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++*launches;
    return e;
}

}  // namespace ptss
