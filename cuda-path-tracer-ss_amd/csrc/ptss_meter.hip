// ptss_meter.hip — the kernels behind ptss_meter_linear, ptss_meter_splat and ptss_meter_exposure (include/ptss.h): a
// luminance histogram of a linear or a filtered linear film and the exposure it asks for, kept in device memory (csrc/ptmeter.h has the
// arithmetic; its host build is the specification). The two resolves that read their exposure from there, ptss_resolve_linear_metered and
// ptss_resolve_splat_metered, are instantiations of ptss_resolve.hip's kernel.
//
//   meterKernel            one streaming read of the film, 32 B per pixel as the two 16-byte rows the resolves read. The grid is capped
//                          (ptmeter::kGridCap workgroups) and strides the range; a workgroup counts into 329 words of LDS and flushes its
//                          non-zero bins with one 32-bit global atomic each — no global atomic per pixel. The counts are integers: every
//                          form of the LDS step, every grid and every split of the range leaves the same bytes
//   meterExposureKernel    one wave takes ptmeter::update's integer sums bin-parallel, lane 0 runs its float steps on the state in place
//
// How a wave's lanes reach the LDS bins has three forms (kFormAtomic, kFormRuns, kFormDistinct); DESIGN.md §3.31 has their timings and
// why kMeterForm is the one the library ships. The other two are compiled in measurement builds only (PTSS_TUNING_KNOBS).
#include "ptss_device.h"
#include "ptfilm.h"
#include "ptmeter.h"

#ifdef PTSS_TUNING_KNOBS
#include <cstdlib>
#endif

namespace ptss {

using ptlin::u64;

constexpr int kMeterBlock = ptmeter::kBlock;   // the histogram kernels: sixteen waves share one LDS histogram and one flush
constexpr int kMeterBins = ptmeter::kBins;
constexpr int kFormAtomic = 0;                        // a. every metered lane: one LDS atomic on its bin
[[maybe_unused]] constexpr int kFormRuns = 1;       // b. neighbouring lanes with one bin summed first (sumRunsToHead), the run's head alone adds
[[maybe_unused]] constexpr int kFormDistinct = 2;   // c. a loop over the wave's distinct bins: first-lane broadcast, ballot, one add of the popcount
constexpr int kMeterForm = kFormAtomic;

// one trip of a wave: `bin` is the lane's own, ptmeter::kNoBin where it has no pixel to meter. Every lane of the wave takes part
template <int Form>
__device__ __forceinline__ void countBins(uint32_t* sBins, int bin) {
    const bool metered = bin != ptmeter::kNoBin;
    if (Form == kFormAtomic) {
        if (metered) atomicAdd(&sBins[bin], 1u);
    } else if (Form == kFormRuns) {
        uint32_t n = metered ? 1u : 0u;
        const bool head = sumRunsToHead((uint32_t)bin, [&](uint32_t d, bool joins) {
            const uint32_t n2 = (uint32_t)__shfl_down((int)n, d, 64);
            if (joins) n += n2;
        });
        if (head && metered) atomicAdd(&sBins[bin], n);
    } else {
        unsigned long long todo = __builtin_amdgcn_ballot_w64(metered);
        const uint32_t lane = laneId();
        while (todo != 0ull) {   // (wave-uniform: todo is a ballot)
            const uint32_t first = (uint32_t)__builtin_ctzll(todo);
            const int b = __shfl(bin, (int)first, 64);
            const unsigned long long same = __builtin_amdgcn_ballot_w64(bin == b);   // (b is a metered lane's: kNoBin never matches)
            if (lane == first) atomicAdd(&sBins[b], (uint32_t)__popcll(same));
            todo &= ~same;
        }
    }
}

// Splat: the film is ptss_splat_entry (word 3 the summed weight), else ptss_linear_entry (its low half the samples)
template <int Form, bool Splat>
__global__ __launch_bounds__(kMeterBlock) void meterKernel(const ulonglong2* __restrict__ film, uint32_t firstPixel, uint32_t count,
                                                           uint32_t* __restrict__ histogram) {
    __shared__ uint32_t sBins[kMeterBins];
    for (int b = (int)threadIdx.x; b < kMeterBins; b += kMeterBlock) sBins[b] = 0u;
    __syncthreads();
    const uint32_t stride = gridDim.x * kMeterBlock;   // at most 2^18; base < count < 2^31: base + stride does not wrap
    for (uint32_t base = blockIdx.x * kMeterBlock; base < count; base += stride) {   // (every lane takes every trip: the forms are wave-wide)
        const uint32_t i = base + threadIdx.x;
        int bin = ptmeter::kNoBin;
        if (i < count) {
            const size_t p = (size_t)firstPixel + i;
            const ulonglong2 rg = film[2 * p], bw = film[2 * p + 1];
            bin = Splat ? ptmeter::binOfSplat(rg.x, rg.y, bw.x, bw.y) : ptmeter::binOfLinear(rg.x, rg.y, bw.x, (uint32_t)bw.y);
        }
        countBins<Form>(sBins, bin);
    }
    __syncthreads();
    for (int b = (int)threadIdx.x; b < kMeterBins; b += kMeterBlock) {
        const uint32_t n = sBins[b];
        if (n != 0u) atomicAdd(histogram + b, n);
    }
}

// One wave. ptmeter::update's integers are sums of integers, so the wave takes them bin-parallel: lane l holds bins 1 + 6 l .. 6 + 6 l (64
// lanes x 6 >= 328), a scan over the lanes gives every bin the ranks in front of it and T, each lane adds up its bins' binLog, a reduction
// gives sumLog. Lane 0 then runs the float steps (ptmeter::expose) on the state in place. (One lane walking the 328 bins twice, one
// dependent read after another, took 0.035 ms: more than the histogram of a 1080p film.)
constexpr int kBinsPerLane = 6;
static_assert(64 * kBinsPerLane >= kMeterBins - 1, "one wave holds every bin but the black one");

__global__ __launch_bounds__(64) void meterExposureKernel(const uint32_t* __restrict__ histogram, ptmeter::Rule rule, ptss_meter_state* state) {
    const int lane = (int)threadIdx.x;
    u64 mine[kBinsPerLane], local = 0ull;
#pragma unroll
    for (int k = 0; k < kBinsPerLane; ++k) {
        const int b = 1 + lane * kBinsPerLane + k;
        mine[k] = b < kMeterBins ? (u64)histogram[b] : 0ull;
        local += mine[k];
    }
    const u64 upTo = waveScan(local, (uint32_t)lane);   // the counts of this lane's bins and of every lane below
    const u64 T = (u64)__shfl((long long)upTo, 63, 64);
    const u64 lo = ptmeter::lowRank(T, rule), hi = ptmeter::highRank(T, rule);
    u64 before = upTo - local, sumLog = 0ull;
#pragma unroll
    for (int k = 0; k < kBinsPerLane; ++k) {
        sumLog += ptmeter::binLog(1 + lane * kBinsPerLane + k, before, mine[k], lo, hi);   // (a bin beyond the histogram holds no rank: it adds 0)
        before += mine[k];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sumLog += (u64)__shfl_down((long long)sumLog, d, 64);
    if (lane != 0) return;
    ptss_meter_state s = *state;
    ptmeter::expose((u64)histogram[0], T, T != 0ull ? hi - lo : 0ull, sumLog, rule, &s);
    *state = s;
}

template <int Form>
static void launchMeterForm(hipStream_t st, const void* film, bool splat, uint32_t firstPixel, uint32_t count, uint32_t* histogram, unsigned cap) {
    const unsigned blocks = filmBlocksFor(count, kMeterBlock);
    const dim3 grid(blocks < cap ? blocks : cap), block(kMeterBlock);
    if (splat)
        hipLaunchKernelGGL((meterKernel<Form, true>), grid, block, 0, st, static_cast<const ulonglong2*>(film), firstPixel, count, histogram);
    else
        hipLaunchKernelGGL((meterKernel<Form, false>), grid, block, 0, st, static_cast<const ulonglong2*>(film), firstPixel, count, histogram);
}

hipError_t launchMeterHistogram(hipStream_t st, const void* film, bool splat, uint32_t firstPixel, uint32_t count, uint32_t* histogram,
                                unsigned long long* launches) {
    unsigned cap = (unsigned)ptmeter::kGridCap;
#ifdef PTSS_TUNING_KNOBS   // measurement builds only (tools/build_variants.py "knobs"; tools/meter_bench.py); the shipped library reads no environment
    int form = kMeterForm;
    if (const char* e = getenv("PTSS_METER_FORM")) form = atoi(e);
    if (const char* e = getenv("PTSS_METER_GRID_CAP")) cap = atoi(e) > 0 ? (unsigned)atoi(e) : cap;
    if (form == kFormRuns) launchMeterForm<kFormRuns>(st, film, splat, firstPixel, count, histogram, cap);
    else if (form == kFormDistinct) launchMeterForm<kFormDistinct>(st, film, splat, firstPixel, count, histogram, cap);
    else
#endif
        launchMeterForm<kMeterForm>(st, film, splat, firstPixel, count, histogram, cap);
    return counted(launches);
}

hipError_t launchMeterExposure(hipStream_t st, const uint32_t* histogram, const ptss_linear_params& params, const ptss_meter_params& meter,
                               ptss_meter_state* state, unsigned long long* launches) {
    hipLaunchKernelGGL(meterExposureKernel, dim3(1), dim3(64), 0, st, histogram, ptmeter::ruleOf(meter, params), state);
    return counted(launches);
}

}  // namespace ptss
