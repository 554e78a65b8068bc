// ptss_linear.hip — the kernels behind ptss_accumulate_paths_linear and ptss_accumulate_paths_linear_stats (include/ptss.h; DESIGN.md
// §3.29, §3.33): a film that holds linear radiance as 64-bit fixed-point sums, order-free and exact for every index, and beside it, where
// the caller keeps them, the luminance moments of its fixed-point samples (csrc/ptlinear.h and csrc/ptlinstats.h have the arithmetic;
// their host builds are the specification). One pair of kernels writes both: the film's words come from one sequence of source lines in
// every call, so a film accumulated with moments holds the bytes of one accumulated without. The film may be absent: a filtered film
// keeps its moments by home pixel beside ptss_splat_paths. The resolves are ptss_resolve.hip's; the plan that reads the moments
// (ptss_plan_samples_linear) lives beside the scan it shares, in ptss_adaptive.hip.
//
// With an index, the lanes of a wave that hold one pixel side by side are summed on chip first and the run's head lane alone issues the
// atomics (csrc/ptfilm.h sumRunsToHead, the reduction ptss_adaptive.hip uses).
#include "ptss_device.h"
#include "ptfilm.h"
#include "ptlinstats.h"

namespace ptss {

using ptlin::u64;

constexpr int kLinearBlock = 256;

// without an index: ray i belongs to pixel firstPixel + i alone — a plain read-modify-write of the 32-byte entry (kFilm) and of the
// 32-byte moment row (kMoments)
template <bool kFilm, bool kMoments>
__global__ __launch_bounds__(kLinearBlock) void linearAccumulateKernel(const float4* __restrict__ results, uint32_t firstPixel, uint32_t n,
                                                                       ulonglong2* __restrict__ film, ulonglong2* __restrict__ moments,
                                                                       ptlin::Scale sc) {
    static_assert(kFilm || kMoments, "a launch writes a film, moments or both");
    const uint32_t i = blockIdx.x * kLinearBlock + threadIdx.x;
    if (i >= n) return;
    const float4 r = results[i];
    u64 q[3];
    const uint32_t flag = ptlin::sampleToFixed(r.x, r.y, r.z, sc, q);
    [[maybe_unused]] const ptls::Sample s = ptls::sampleOf(q[0], q[1], q[2]);   // (dead without moments)
    const size_t p = (size_t)firstPixel + i;
    if (kMoments) {
        ulonglong2* m = moments + 2 * p;
        ulonglong2 ys = m[0], hn = m[1];
        ys.x += s.y;
        ys.y += s.lo;
        hn.x += s.hi;
        hn.y += 1ull;
        m[0] = ys;
        m[1] = hn;
    }
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

// with an index: the runs of equal, in-range pixels inside a wave are summed by a segmented reduction towards the run's first lane,
// which alone issues the 64-bit atomics: four for the moment row, four for the film. A run is split at the wave's edge, and duplicates
// that are not neighbours meet in the atomics, so the sums are exact for every index. A sample's channels and its y, lo and hi are at
// most 2^40 and a wave's run at most 64 * 2^40 = 2^46: each travels as two 32-bit words; the counts, at most 64 each, share one
// (samples | clamped << 16). Seven words travel with a film or with moments alone, thirteen with both, six steps each.
template <bool kFilm, bool kMoments>
__global__ __launch_bounds__(kLinearBlock) void linearScatterKernel(const float4* __restrict__ results, const uint32_t* __restrict__ index, uint32_t n,
                                                                    u64* __restrict__ film, u64* __restrict__ moments, uint32_t filmPixels,
                                                                    ptlin::Scale sc, unsigned long long* __restrict__ rejected) {
    static_assert(kFilm || kMoments, "a launch writes a film, moments or both");
    const uint32_t i = blockIdx.x * kLinearBlock + threadIdx.x;
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
        if (kMoments) s = ptls::sampleOf(q[0], q[1], q[2]);
    }
    // (the moment's words, the counts, the film's words, and the moments next to the film among the arguments: with another order the
    // kernel with both measured slower on a plan's index; DESIGN.md §3.33, profiles/film_resolve/resolve_ab.txt)
    const bool head = sumRunsToHead(key, [&](uint32_t d, bool joins) {
        u64 r2 = 0ull, g2 = 0ull, b2 = 0ull, y2 = 0ull, lo2 = 0ull, hi2 = 0ull;
        if (kMoments) {
            y2 = (u64)__shfl_down((long long)s.y, d, 64);
            lo2 = (u64)__shfl_down((long long)s.lo, d, 64);
            hi2 = (u64)__shfl_down((long long)s.hi, d, 64);
        }
        const uint32_t c2 = (uint32_t)__shfl_down((int)counts, d, 64);
        if (kFilm) {
            r2 = (u64)__shfl_down((long long)q[0], d, 64);
            g2 = (u64)__shfl_down((long long)q[1], d, 64);
            b2 = (u64)__shfl_down((long long)q[2], d, 64);
        }
        if (joins) {
            if (kMoments) {
                s.y += y2;
                s.lo += lo2;
                s.hi += hi2;
            }
            counts += c2;
            if (kFilm) {
                q[0] += r2;
                q[1] += g2;
                q[2] += b2;
            }
        }
    });
    if (!(head && ok)) return;
    if (kMoments) {
        u64* m = moments + 4 * (size_t)p;
        atomicAdd(m + 0, s.y);
        atomicAdd(m + 1, s.lo);
        atomicAdd(m + 2, s.hi);
        atomicAdd(m + 3, (u64)(counts & 0xffffu));
    }
    if (kFilm) {
        u64* e = film + 4 * (size_t)p;
        atomicAdd(e + 0, q[0]);
        atomicAdd(e + 1, q[1]);
        atomicAdd(e + 2, q[2]);
        atomicAdd(e + 3, (u64)(counts & 0xffffu) | ((u64)(counts >> 16) << 32));   // samples | clamped << 32, one word
    }
}

template <bool kFilm, bool kMoments>
static void launchLinearPair(hipStream_t st, const float4* results, const uint32_t* index, uint32_t firstPixel, uint32_t n, void* film, void* moments,
                             uint32_t filmPixels, ptlin::Scale sc, unsigned long long* rejected) {
    const dim3 grid(filmBlocksFor(n, kLinearBlock)), block(kLinearBlock);
    if (!index)
        hipLaunchKernelGGL((linearAccumulateKernel<kFilm, kMoments>), grid, block, 0, st, results, firstPixel, n, static_cast<ulonglong2*>(film),
                           static_cast<ulonglong2*>(moments), sc);
    else
        hipLaunchKernelGGL((linearScatterKernel<kFilm, kMoments>), grid, block, 0, st, results, index, n, static_cast<u64*>(film),
                           static_cast<u64*>(moments), filmPixels, sc, rejected);
}

hipError_t launchLinearAccumulate(hipStream_t st, const void* results, const uint32_t* index, uint32_t firstPixel, uint32_t n, void* film,
                                  void* moments, uint32_t filmPixels, const ptss_linear_params& params, unsigned long long* rejected,
                                  unsigned long long* launches) {
    const float4* res = static_cast<const float4*>(results);
    const ptlin::Scale sc = ptlin::scaleOf(params);
    if (!moments)
        launchLinearPair<true, false>(st, res, index, firstPixel, n, film, moments, filmPixels, sc, rejected);
    else if (film)
        launchLinearPair<true, true>(st, res, index, firstPixel, n, film, moments, filmPixels, sc, rejected);
    else
        launchLinearPair<false, true>(st, res, index, firstPixel, n, film, moments, filmPixels, sc, rejected);
    return counted(launches);
}

}  // namespace ptss
