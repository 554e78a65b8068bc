// ptss_tone.hip — tone curves for the two linear films: ptss_tone_build and ptss_resolve_toned (include/ptss.h). The
// arithmetic is that of csrc/pttone.h, whose host build is the specification.
//
//   toneBuildKernel      one workgroup, one thread per entry T[0 .. K]: 31 bisection steps of the literal level, the order of the thresholds
//                        checked through LDS, the flag and the padding written by thread 0
//   tonedResolveKernel   ptss_resolve.hip's streaming pass (two 16-byte reads of the entry, up to three stores) with the mean shown through a
//                        tone rule: over the film's kind, over glare (four taps of u_1 in front of the curve), over the bit depth and over
//                        the form of the lookup. A meter's state is tested at run time: it is one kernel argument, the same for all lanes.
//                        A workgroup of 256 threads shows kTonePixels pixels, thread t pixels t, t + 256, ..
//
// The lookup, three per pixel, in two forms that give levelCount's number for every input:
//   kFormStaged   T[0 .. K] copied into LDS once per workgroup (1 or 4 KiB, float4 rows), then pttone::levelSearch: 8 or 10 steps without a
//                 branch. The first steps read one address for the whole wave (a broadcast); the last ones scatter over the banks
//   kFormGuess    a first guess from the exact curve and the hardware log2 / exp2 of the transfer, as ptq::quantize_fast takes one, settled by
//                 pttone::levelSettle against the table in global memory: right for any guess, one or two comparisons for a good one
#include "ptss_device.h"
#include "ptfilm.h"
#include "pttone.h"

namespace ptss {

using ptlin::u64;

constexpr int kToneBlock = 256;
constexpr int kTonePerThread = 4;
constexpr int kTonePixels = kToneBlock * kTonePerThread;
constexpr int kFormStaged = 1, kFormGuess = 2;
constexpr int kFormShipped = kFormStaged;   // DESIGN.md §3.37 has the measurement

template <int Threads>
__global__ __launch_bounds__(Threads) void toneBuildKernel(pttone::Stage S, float* __restrict__ table) {
    __shared__ float sT[Threads];
    const uint32_t k = threadIdx.x, K = (uint32_t)Threads - 1u;   // the launch has Threads = K + 1
    const float t = k == 0u ? pttone::fixedEntry(0u) : pttone::thresholdOf(S, k);
    sT[k] = t;
    __syncthreads();
    const bool outOfOrder = k >= 2u && !pttone::inOrder(sT[k - 1u], t);
    const int unsorted = __syncthreads_or(outOfOrder ? 1 : 0);
    table[k] = t;
    if (k == 0u) {
        table[K + 1u] = pttone::fixedEntry(K + 1u);
        table[K + 2u] = unsorted ? 1.f : 0.f;
        table[K + 3u] = pttone::fixedEntry(K + 3u);
        table[K + 4u] = pttone::fixedEntry(K + 4u);
    }
}

// what the toned resolve takes besides the film and the tone rule; the glare's fields are read by the glare instantiations only
struct TonedSource {
    ptlin::Scale sc;
    const ptss_meter_state* state;   // or null
    int width;                       // of the film
    int cw, ch;                      // level 1
    ptglare::Rule rule;
    const ulonglong2* u1;
};

// the guess of kFormGuess: the level of x from the exact curve and the approximate transfer, somewhere in 0 .. K for every input
template <uint32_t K>
__device__ __forceinline__ uint32_t guessLevel(const pttone::Stage& S, float x) {
    const float c = pttone::curveOf(S, x);
    const float p = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(c) * (S.transfer == PTSS_TRANSFER_SRGB ? pttone::kSrgbPower : ptm::kGamma));
    const float v = S.transfer == PTSS_TRANSFER_SRGB ? (c <= pttone::kSrgbKnee ? pttone::kSrgbSlope * c : __builtin_fmaf(pttone::kSrgbScale, p, pttone::kSrgbOffset)) : p;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_fmed3f(__builtin_fmaf((float)K, v, 0.5f), 0.0f, (float)K);
    return k0 > K ? K : k0;   // whatever a NaN converts to, the index stays in the table
}

template <bool Splat, bool Glare, int Bits, int Form>
__global__ __launch_bounds__(kToneBlock) void tonedResolveKernel(const ulonglong2* __restrict__ film, uint32_t firstPixel, uint32_t count, TonedSource src,
                                                                 pttone::Rule R, const float* __restrict__ table, float4* __restrict__ linear,
                                                                 uint32_t* __restrict__ pixels, float4* __restrict__ history) {
    constexpr uint32_t K = Bits == 10 ? 1023u : 255u;
    __shared__ __attribute__((aligned(16))) float sT[Form == kFormStaged ? K + 1u : 4u];
    if constexpr (Form == kFormStaged) {
        for (uint32_t row = threadIdx.x; row < (K + 1u) / 4u; row += kToneBlock)
            reinterpret_cast<float4*>(sT)[row] = reinterpret_cast<const float4*>(table)[row];
        __syncthreads();
    }
    ptlin::Scale sc = src.sc;
    if (src.state) sc.exposure = src.state->exposure * sc.exposure;
    auto levelOf = [&](float x) -> uint32_t {
        if constexpr (Form == kFormStaged)
            return pttone::levelSearch(sT, K, x);
        else
            return pttone::levelSettle(table, K, x, guessLevel<K>(R.shown, x));
    };
    const uint32_t first = blockIdx.x * (uint32_t)kTonePixels + threadIdx.x;   // below count + kTonePixels < 2^32
    for (int j = 0; j < kTonePerThread; ++j) {
        const uint32_t i = first + (uint32_t)(j * kToneBlock);
        if (i >= count) break;   // no barrier follows
        const uint32_t p = firstPixel + i;
        [[maybe_unused]] u64 up[3];
        if constexpr (Glare) {
            const int y = (int)(p / (uint32_t)src.width), x = (int)(p - (uint32_t)y * (uint32_t)src.width);
            ptglare::upTexel(x, y, src.cw, src.ch, [&](int ci, int cj, u64* v) { loadEntry(src.u1, (size_t)cj * (size_t)src.cw + (size_t)ci, v); }, up);
        }
        const ulonglong2 rg = film[2 * (size_t)p], bw = film[2 * (size_t)p + 1];
        float lin[4], hist[4];
        uint32_t px;
        pttone::resolve(rg.x, rg.y, bw.x, Splat ? bw.y : (bw.y & 0xffffffffull), Splat, Glare ? up : nullptr, &src.rule, sc, R, levelOf, lin, &px, hist);
        if (linear) linear[p] = float4{lin[0], lin[1], lin[2], lin[3]};
        if (pixels) pixels[p] = px;
        if (history) history[p] = float4{hist[0], hist[1], hist[2], hist[3]};
    }
}

hipError_t launchToneBuild(hipStream_t st, const ptss_tone_params& tone, float* table, unsigned long long* launches) {
    const pttone::Stage S = pttone::ruleOf(tone).shown;
    if (tone.bits == 10)
        hipLaunchKernelGGL(toneBuildKernel<1024>, dim3(1), dim3(1024), 0, st, S, table);
    else
        hipLaunchKernelGGL(toneBuildKernel<256>, dim3(1), dim3(256), 0, st, S, table);
    return counted(launches);
}

template <bool Splat, bool Glare, int Bits>
static void launchTonedForm(hipStream_t st, int form, dim3 grid, const ulonglong2* f, uint32_t firstPixel, uint32_t count, const TonedSource& src,
                            const pttone::Rule& R, const float* table, float4* lin, uint32_t* pixels, float4* hist) {
    if (form == kFormGuess)
        hipLaunchKernelGGL((tonedResolveKernel<Splat, Glare, Bits, kFormGuess>), grid, dim3(kToneBlock), 0, st, f, firstPixel, count, src, R, table, lin, pixels, hist);
    else
        hipLaunchKernelGGL((tonedResolveKernel<Splat, Glare, Bits, kFormStaged>), grid, dim3(kToneBlock), 0, st, f, firstPixel, count, src, R, table, lin, pixels, hist);
}

hipError_t launchTonedResolve(hipStream_t st, const void* film, bool splat, uint32_t firstPixel, uint32_t count, const ptss_linear_params& params,
                              const ptss_tone_params& tone, const float* table, const ptss_meter_state* state, const GlareResolveArgs* glare, int form,
                              void* linear, uint32_t* pixels, void* history, unsigned long long* launches) {
    TonedSource src{};
    src.sc = ptlin::scaleOf(params);
    src.state = state;
    if (glare) {
        src.width = glare->width;
        src.cw = ptglare::halfOf(glare->width), src.ch = ptglare::halfOf(glare->height);
        src.rule = ptglare::ruleOf(*glare->params, params);
        src.u1 = static_cast<const ulonglong2*>(glare->pyramid);
    }
    const pttone::Rule R = pttone::ruleOf(tone);
    const int chosen = form == 0 ? kFormShipped : form;
    const dim3 grid(filmBlocksFor(count, kTonePixels));
    const ulonglong2* f = static_cast<const ulonglong2*>(film);
    float4 *lin = static_cast<float4*>(linear), *hist = static_cast<float4*>(history);
    auto pick = [&](auto splatC, auto glareC) {
        if (tone.bits == 10)
            launchTonedForm<decltype(splatC)::value, decltype(glareC)::value, 10>(st, chosen, grid, f, firstPixel, count, src, R, table, lin, pixels, hist);
        else
            launchTonedForm<decltype(splatC)::value, decltype(glareC)::value, 8>(st, chosen, grid, f, firstPixel, count, src, R, table, lin, pixels, hist);
    };
    using T = std::true_type;
    using F = std::false_type;
    if (splat) {
        if (glare) pick(T{}, T{}); else pick(T{}, F{});
    } else {
        if (glare) pick(F{}, T{}); else pick(F{}, F{});
    }
    return counted(launches);
}

}  // namespace ptss
