// ptss_adaptive.hip — the kernels behind ptss_accumulate_paths_stats and ptss_plan_samples (include/ptss.h): a film
// that also keeps the second moment of its tone-mapped samples, and the plan that turns film and moments into the next round's index
// without a host round trip (csrc/ptadaptive.h has the arithmetic; its host build is the specification).
//
// The accumulate kernels write the bytes the kernels of ptss_film.hip write (the same ptq::quantize_fast, the same table, the same
// resolveEntry: csrc/ptfilm.h). With an index, the lanes of a wave that hold one pixel side by side — a plan's index is sorted, so all
// of them do — are summed on chip first (ptfilm.h sumRunsToHead) and the run's head lane alone issues the atomics.
//
// The plan is one scan with two weight sources: reduce / scan of the tile sums / downsweep — three launches, no workgroup waits for
// another — and the index. The weight is computed inside both loads; no weight array exists. PlanArgs takes it from the 8-bit film and
// its moments (ptss_plan_samples), LinPlanArgs from the linear film's moments (ptss_plan_samples_linear; csrc/ptlinstats.h; DESIGN.md
// §3.33): the reduce and the downsweep are templates on the two, the tile sums and the index kernel never see a weight.
#include "ptss_device.h"
#include "ptadaptive.h"
#include "ptfilm.h"
#include "ptquant.h"
#include "ptlinstats.h"

namespace ptss {

using ptad::u64;

constexpr int kStatsBlock = 256;
constexpr int kScanBlock = 256;
constexpr int kScanPerLane = ptad::kScanTile / kScanBlock;   // 8 pixels per lane, 64 apart inside a wave's 512
constexpr int kScanWaves = kScanBlock / 64;
constexpr int kSumsBlock = 1024;                             // the one workgroup that scans the tile sums
static_assert(kScanPerLane * kScanBlock == ptad::kScanTile && kScanBlock % 64 == 0, "a tile is whole waves of whole rounds");

// without an index: ray i belongs to pixel firstPixel + i alone — a plain read-modify-write of the entry and of the moment
__global__ __launch_bounds__(kStatsBlock) void statsAccumulateKernel(const float4* __restrict__ results, uint32_t firstPixel, uint32_t n,
                                                                     uint4* __restrict__ film, u64* __restrict__ moments,
                                                                     ptss_uchar4* __restrict__ pixels, float4* __restrict__ history,
                                                                     const float* __restrict__ quantT) {
    const uint32_t i = blockIdx.x * kStatsBlock + threadIdx.x;
    if (i >= n) return;
    const float4 r = results[i];
    const uint32_t p = firstPixel + i;
    const uint32_t qr = ptq::quantize_fast(r.x, quantT), qg = ptq::quantize_fast(r.y, quantT), qb = ptq::quantize_fast(r.z, quantT);
    uint4 e = film[p];
    e.x += qr;
    e.y += qg;
    e.z += qb;
    e.w += 1u;
    film[p] = e;
    moments[p] += (u64)ptad::squares(qr, qg, qb);
    resolveEntry(e, p, pixels, history);
}

// with an index: the runs of equal, in-range pixels inside a wave are summed by a segmented reduction towards the run's first lane,
// which alone issues the atomics (four 32-bit, one 64-bit). A run is split at the wave's edge, and duplicates that are not neighbours
// meet in the atomics, so the sums are exact for every index. 64 samples of a wave fit 16 bits per channel (64 * 255) and 32 bits of
// squares (64 * 195,075): three words travel — r | g << 16, b | count << 16, the squares.
__global__ __launch_bounds__(kStatsBlock) void statsScatterKernel(const float4* __restrict__ results, const uint32_t* __restrict__ index, uint32_t n,
                                                                  uint32_t* __restrict__ film, u64* __restrict__ moments, uint32_t filmPixels,
                                                                  const float* __restrict__ quantT, unsigned long long* __restrict__ rejected) {
    const uint32_t i = blockIdx.x * kStatsBlock + threadIdx.x;
    const bool inBatch = i < n;
    const uint32_t p = inBatch ? index[i] : 0u;
    const bool ok = inBatch && p < filmPixels;
    countDropped(inBatch && !ok, rejected);
    const uint32_t key = ok ? p : 0xffffffffu;   // (a film has fewer than 2^31 pixels) lanes without a pixel carry zeros and never lead a store
    uint32_t rg = 0u, bc = 0u, sq = 0u;
    if (ok) {
        const float4 r = results[i];
        const uint32_t qr = ptq::quantize_fast(r.x, quantT), qg = ptq::quantize_fast(r.y, quantT), qb = ptq::quantize_fast(r.z, quantT);
        rg = qr | (qg << 16);
        bc = qb | (1u << 16);
        sq = ptad::squares(qr, qg, qb);
    }
    const bool head = sumRunsToHead(key, [&](uint32_t d, bool joins) {
        const uint32_t rg2 = (uint32_t)__shfl_down((int)rg, d, 64), bc2 = (uint32_t)__shfl_down((int)bc, d, 64),
                       sq2 = (uint32_t)__shfl_down((int)sq, d, 64);
        if (joins) {
            rg += rg2;
            bc += bc2;
            sq += sq2;
        }
    });
    if (!(head && ok)) return;
    uint32_t* e = film + 4 * (size_t)p;
    atomicAdd(e + 0, rg & 0xffffu);
    atomicAdd(e + 1, rg >> 16);
    atomicAdd(e + 2, bc & 0xffffu);
    atomicAdd(e + 3, bc >> 16);
    atomicAdd(moments + p, (unsigned long long)sq);
}

// every run of the index resolves its pixel once per wave; runs that share a pixel store the same bytes
__global__ __launch_bounds__(kStatsBlock) void statsResolveKernel(const uint32_t* __restrict__ index, uint32_t n, const uint4* __restrict__ film,
                                                                  uint32_t filmPixels, ptss_uchar4* __restrict__ pixels,
                                                                  float4* __restrict__ history) {
    const uint32_t i = blockIdx.x * kStatsBlock + threadIdx.x;
    const uint32_t p = i < n ? index[i] : 0xffffffffu;
    const uint32_t before = (uint32_t)__shfl_up((int)p, 1, 64);
    if (p >= filmPixels || (laneId() != 0u && p == before)) return;
    resolveEntry(film[p], p, pixels, history);
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------------
// What a plan reads, and the weight of pixel p < filmPixels from it (a weight is at most 2^19 in both; `kind`: ptad::kActive ..)
struct PlanArgs {
    const uint4* film;
    const u64* moments;
    uint32_t filmPixels;
    uint32_t minSamples, maxSamples;
    float threshold;
    __device__ __forceinline__ uint32_t weight(uint32_t p, uint32_t* kind) const {
        const uint4 e = film[p];
        return ptad::weight(e.x, e.y, e.z, e.w, moments[p], minSamples, maxSamples, threshold, kind);
    }
};

struct LinPlanArgs {
    const ulonglong2* moments;   // a row as the two 16-byte halves it is read in: {sumY, sqLo}, {sqHi, samples}
    uint32_t filmPixels;
    ptls::Rule rule;
    __device__ __forceinline__ uint32_t weight(uint32_t p, uint32_t* kind) const {
        const ulonglong2 ys = moments[2 * (size_t)p], hn = moments[2 * (size_t)p + 1];
        return ptls::weight(ys.x, ys.y, hn.x, hn.y, rule, kind);
    }
};

// the weight of pixel p (0 beyond the film), its kind added to the three counters
template <class Args>
__device__ __forceinline__ uint32_t loadWeight(const Args& a, uint32_t p, uint32_t& active, uint32_t& unsampled, uint32_t& capped) {
    if (p >= a.filmPixels) return 0u;
    uint32_t kind;
    const uint32_t w = a.weight(p, &kind);
    active += kind & ptad::kActive ? 1u : 0u;
    unsampled += kind & ptad::kUnsampled ? 1u : 0u;
    capped += kind & ptad::kCapped ? 1u : 0u;
    return w;
}

// pixel k of lane `lane` of wave `wave` of tile `tile`: a wave owns 512 consecutive pixels, a round of it 64
__device__ __forceinline__ uint32_t scanPixel(uint32_t tile, uint32_t wave, uint32_t k, uint32_t lane) {
    return tile * (uint32_t)ptad::kScanTile + wave * (64u * kScanPerLane) + k * 64u + lane;   // < 2^31 + 2048
}

// step 1: the sum of a tile's weights (at most 2048 * 2^19 = 2^30) and its three counts -> work[3 tile .. 3 tile + 2]
template <class Args>
__global__ __launch_bounds__(kScanBlock) void planReduceKernel(Args a, u64* __restrict__ work) {
    __shared__ uint32_t part[kScanWaves][4];
    const uint32_t lane = laneId(), wave = threadIdx.x / 64u;
    uint32_t sum = 0u, active = 0u, unsampled = 0u, capped = 0u;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kScanPerLane; ++k) sum += loadWeight(a, scanPixel(blockIdx.x, wave, k, lane), active, unsampled, capped);
    sum = waveSum(sum);
    active = waveSum(active);
    unsampled = waveSum(unsampled);
    capped = waveSum(capped);
    if (lane == 0u) {
        part[wave][0] = sum;
        part[wave][1] = active;
        part[wave][2] = unsampled;
        part[wave][3] = capped;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t t[4] = {0u, 0u, 0u, 0u};
        for (int w = 0; w < kScanWaves; ++w)
            for (int c = 0; c < 4; ++c) t[c] += part[w][c];
        u64* out = work + (size_t)ptad::kWorkspacePerTile * blockIdx.x;
        out[0] = (u64)t[0];
        out[1] = (u64)t[1] | ((u64)t[2] << 32);
        out[2] = (u64)t[3];
    }
}

// step 2, one workgroup: the tile sums become the sums of the tiles in front of each (exclusive), 1024 tiles per pass with a carry;
// the totals go to *info
__global__ __launch_bounds__(kSumsBlock) void planTileSumsKernel(u64* __restrict__ work, uint32_t tiles, ptss_plan_info* __restrict__ info) {
    __shared__ u64 waveTotal[kSumsBlock / 64];
    __shared__ u64 counts[3];
    const uint32_t lane = laneId(), wave = threadIdx.x / 64u;
    if (threadIdx.x < 3u) counts[threadIdx.x] = 0ull;
    u64 carry = 0ull;
    u64 active = 0ull, unsampled = 0ull, capped = 0ull;
    for (uint32_t base = 0u; base < tiles; base += (uint32_t)kSumsBlock) {   // (uniform bounds: every lane takes every pass)
        const uint32_t t = base + threadIdx.x;
        u64* w = work + (size_t)ptad::kWorkspacePerTile * t;
        u64 own = 0ull;
        if (t < tiles) {
            own = w[0];
            active += w[1] & 0xffffffffull;
            unsampled += w[1] >> 32;
            capped += w[2];
        }
        u64 v = own;   // inclusive over the wave (written out: through ptfilm.h's waveScan the same instructions come out in another order)
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const u64 o = (u64)__shfl_up((long long)v, d, 64);
            if (lane >= d) v += o;
        }
        __syncthreads();   // the previous pass has read waveTotal
        if (lane == 63u) waveTotal[wave] = v;
        __syncthreads();
        u64 front = carry, all = carry;
        for (uint32_t k = 0u; k < (uint32_t)(kSumsBlock / 64); ++k) {
            if (k < wave) front += waveTotal[k];
            all += waveTotal[k];
        }
        if (t < tiles) w[0] = front + v - own;
        carry = all;
    }
    if (!info) return;
    __syncthreads();
    atomicAdd(&counts[0], active);   // LDS atomics: integer, exact in any order
    atomicAdd(&counts[1], unsampled);
    atomicAdd(&counts[2], capped);
    __syncthreads();
    if (threadIdx.x == 0u) {
        info->totalWeight = carry;
        info->activePixels = (uint32_t)counts[0];
        info->unsampledPixels = (uint32_t)counts[1];
        info->cappedPixels = (uint32_t)counts[2];
        info->uniform = carry == 0ull ? 1u : 0u;
        info->reserved[0] = info->reserved[1] = 0u;
    }
}

// step 3: the weights again, scanned inside the tile (32-bit: a tile's sum is at most 2^30) on top of the sum of the tiles in front
template <class Args>
__global__ __launch_bounds__(kScanBlock) void planDownsweepKernel(Args a, const u64* __restrict__ work, u64* __restrict__ cdf) {
    __shared__ uint32_t waveTotal[kScanWaves];
    const uint32_t lane = laneId(), wave = threadIdx.x / 64u;
    uint32_t incl[kScanPerLane];
    uint32_t running = 0u, unused0 = 0u, unused1 = 0u, unused2 = 0u;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kScanPerLane; ++k) {
        const uint32_t w = loadWeight(a, scanPixel(blockIdx.x, wave, k, lane), unused0, unused1, unused2);
        incl[k] = running + waveScan(w, lane);
        running = (uint32_t)__shfl((int)incl[k], 63, 64);   // the wave's sum so far
    }
    if (lane == 0u) waveTotal[wave] = running;
    __syncthreads();
    u64 front = work[(size_t)ptad::kWorkspacePerTile * blockIdx.x];
    for (uint32_t k = 0u; k < wave; ++k) front += (u64)waveTotal[k];
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kScanPerLane; ++k) {
        const uint32_t p = scanPixel(blockIdx.x, wave, k, lane);
        if (p < a.filmPixels) cdf[p] = front + (u64)incl[k];
    }
}

// step 4: entry i names the pixel under its target; neighbouring lanes search neighbouring targets
__global__ __launch_bounds__(kStatsBlock) void planIndexKernel(const u64* __restrict__ cdf, uint32_t filmPixels, uint32_t n, uint32_t* __restrict__ index) {
    const uint32_t i = blockIdx.x * kStatsBlock + threadIdx.x;
    if (i >= n) return;
    const u64 total = cdf[filmPixels - 1u];
    index[i] = total == 0ull ? ptad::uniformPixel((u64)i, (u64)n, (u64)filmPixels)
                             : ptad::pixelOf(cdf, filmPixels, ptad::target((u64)i, (u64)n, total));
}

hipError_t launchStatsAccumulate(hipStream_t st, const void* results, const uint32_t* index, uint32_t firstPixel, uint32_t n, void* film,
                                 unsigned long long* moments, uint32_t filmPixels, ptss_uchar4* pixels, void* history, const float* quantTable,
                                 unsigned long long* rejected, unsigned long long* launches) {
    const dim3 grid(filmBlocksFor(n, kStatsBlock)), block(kStatsBlock);
    if (!index) {
        hipLaunchKernelGGL(statsAccumulateKernel, grid, block, 0, st, static_cast<const float4*>(results), firstPixel, n, static_cast<uint4*>(film),
                           moments, pixels, static_cast<float4*>(history), quantTable);
    } else {
        hipLaunchKernelGGL(statsScatterKernel, grid, block, 0, st, static_cast<const float4*>(results), index, n, static_cast<uint32_t*>(film),
                           moments, filmPixels, quantTable, rejected);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (pixels || history)
            hipLaunchKernelGGL(statsResolveKernel, grid, block, 0, st, index, n, static_cast<const uint4*>(film), filmPixels, pixels,
                               static_cast<float4*>(history));
    }
    return counted(launches);
}

// the four launches of a plan; `a` says where the weights come from
template <class Args>
static hipError_t launchPlan(hipStream_t st, const Args& a, uint32_t filmPixels, uint32_t n, u64* cdf, uint32_t* index, ptss_plan_info* info,
                             unsigned long long* launches) {
    const uint32_t tiles = (uint32_t)ptad::scanTiles(filmPixels);
    u64* work = cdf + filmPixels;   // the entries behind the film's own: kWorkspacePerTile words per tile
    hipLaunchKernelGGL(planReduceKernel<Args>, dim3(tiles), dim3(kScanBlock), 0, st, a, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(planTileSumsKernel, dim3(1), dim3(kSumsBlock), 0, st, work, tiles, info);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(planDownsweepKernel<Args>, dim3(tiles), dim3(kScanBlock), 0, st, a, static_cast<const u64*>(work), cdf);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(planIndexKernel, dim3(filmBlocksFor(n, kStatsBlock)), dim3(kStatsBlock), 0, st, static_cast<const u64*>(cdf), filmPixels, n, index);
    return counted(launches);
}

hipError_t launchPlanSamples(hipStream_t st, const void* film, const unsigned long long* moments, uint32_t filmPixels,
                             const ptss_plan_params& params, uint32_t n, unsigned long long* cdf, uint32_t* index, ptss_plan_info* info,
                             unsigned long long* launches) {
    const PlanArgs a{static_cast<const uint4*>(film), moments, filmPixels, params.minSamples, params.maxSamples, params.threshold};
    return launchPlan(st, a, filmPixels, n, cdf, index, info, launches);
}

hipError_t launchPlanSamplesLinear(hipStream_t st, const void* moments, uint32_t filmPixels, const ptss_linear_params& film,
                                   const ptss_linear_plan_params& params, uint32_t n, unsigned long long* cdf, uint32_t* index,
                                   ptss_plan_info* info, unsigned long long* launches) {
    const LinPlanArgs a{static_cast<const ulonglong2*>(moments), filmPixels, ptls::ruleOf(params, film)};
    return launchPlan(st, a, filmPixels, n, cdf, index, info, launches);
}

}  // namespace ptss
