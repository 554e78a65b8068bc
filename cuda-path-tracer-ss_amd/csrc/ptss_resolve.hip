// ptss_resolve.hip — the one kernel behind the six resolves of the two linear films: ptss_resolve_linear, ptss_resolve_splat, their
// _metered and their _glare forms (include/ptss.h). One streaming pass over pixels firstPixel .. firstPixel +
// count: two 16-byte reads of the entry, the shown mean, and up to three stores — linear means, display pixels, history entries, each of
// which may be absent. The template is over the film's kind (ptss_linear_entry, or ptss_splat_entry with the summed weight in word 3) and
// over the source of the shown mean:
//
//   PlainSource     ptlin::resolve / ptspl::resolve at the caller's Scale
//   MeteredSource   the same with Scale.exposure = state->exposure * params.exposure; the state is read unconditionally
//   GlareSource     ptglare::resolve with four taps of u_1 (up(u_1) at the pixel) in front of the tone map; a state's exposure or none,
//                   tested at run time
//
// The arithmetic is that of csrc/ptlinear.h, ptsplat.h and ptglare.h, whose host builds are the specification. A source is one kernel
// argument, so an instantiation takes only what it uses.
#include "ptss_device.h"
#include "ptfilm.h"
#include "ptglare.h"

namespace ptss {

using ptlin::u64;

constexpr int kResolveBlock = 256;

// what a source adds to the kernel's arguments; kMetered: it reads its state's exposure, kGlare: it adds the glare, under a state's exposure if it has one
struct PlainSource {
    static constexpr bool kMetered = false, kGlare = false;
    ptlin::Scale sc;
};

struct MeteredSource {
    static constexpr bool kMetered = true, kGlare = false;
    ptlin::Scale sc;
    const ptss_meter_state* state;   // never null
};

struct GlareSource {
    static constexpr bool kMetered = false, kGlare = true;
    ptlin::Scale sc;
    int width;    // of the film
    int cw, ch;   // level 1
    ptglare::Rule rule;
    const ulonglong2* u1;
    const ptss_meter_state* state;   // or null
};

template <bool Splat, class Source>
__global__ __launch_bounds__(kResolveBlock) void linearFilmResolveKernel(const ulonglong2* __restrict__ film, uint32_t firstPixel, uint32_t count, Source src,
                                                                         const float* __restrict__ quantT, float4* __restrict__ linear,
                                                                         ptss_uchar4* __restrict__ pixels, float4* __restrict__ history) {
    const uint32_t i = blockIdx.x * kResolveBlock + threadIdx.x;
    if (i >= count) return;
    ptlin::Scale sc = src.sc;
    if constexpr (Source::kMetered) sc.exposure = src.state->exposure * sc.exposure;
    if constexpr (Source::kGlare) {
        if (src.state) sc.exposure = src.state->exposure * sc.exposure;
    }
    const uint32_t p = firstPixel + i;
    [[maybe_unused]] u64 up[3];
    if constexpr (Source::kGlare) {
        const int y = (int)(p / (uint32_t)src.width), x = (int)(p - (uint32_t)y * (uint32_t)src.width);
        ptglare::upTexel(x, y, src.cw, src.ch, [&](int ci, int cj, u64* v) { loadEntry(src.u1, (size_t)cj * (size_t)src.cw + (size_t)ci, v); }, up);
    }
    const ulonglong2 rg = film[2 * (size_t)p], bw = film[2 * (size_t)p + 1];
    float lin[4], hist[4];
    uint32_t px;
    if constexpr (Source::kGlare)
        ptglare::resolve(rg.x, rg.y, bw.x, Splat ? bw.y : (bw.y & 0xffffffffull), Splat, up, src.rule, sc, quantT, lin, &px, hist);
    else if (Splat)
        ptspl::resolve(rg.x, rg.y, bw.x, bw.y, sc, quantT, lin, &px, hist);
    else
        ptlin::resolve(rg.x, rg.y, bw.x, (uint32_t)bw.y, sc, quantT, lin, &px, hist);
    if (linear) linear[p] = float4{lin[0], lin[1], lin[2], lin[3]};
    if (pixels) reinterpret_cast<uint32_t*>(pixels)[p] = px;   // uchar4 {x, y, z, w = 255}
    if (history) history[p] = float4{hist[0], hist[1], hist[2], hist[3]};
}

hipError_t launchLinearFilmResolve(hipStream_t st, const void* film, bool splat, uint32_t firstPixel, uint32_t count, const ptss_linear_params& params,
                                   const ptss_meter_state* state, const GlareResolveArgs* glare, const float* quantTable, void* linear,
                                   ptss_uchar4* pixels, void* history, unsigned long long* launches) {
    const ptlin::Scale sc = ptlin::scaleOf(params);
    auto launch = [&](auto src) {
        const dim3 grid(filmBlocksFor(count, kResolveBlock)), block(kResolveBlock);
        const ulonglong2* f = static_cast<const ulonglong2*>(film);
        float4 *lin = static_cast<float4*>(linear), *hist = static_cast<float4*>(history);
        if (splat)
            hipLaunchKernelGGL((linearFilmResolveKernel<true, decltype(src)>), grid, block, 0, st, f, firstPixel, count, src, quantTable, lin, pixels, hist);
        else
            hipLaunchKernelGGL((linearFilmResolveKernel<false, decltype(src)>), grid, block, 0, st, f, firstPixel, count, src, quantTable, lin, pixels, hist);
    };
    if (glare)
        launch(GlareSource{sc, glare->width, ptglare::halfOf(glare->width), ptglare::halfOf(glare->height), ptglare::ruleOf(*glare->params, params),
                           static_cast<const ulonglong2*>(glare->pyramid), state});
    else if (state)
        launch(MeteredSource{sc, state});
    else
        launch(PlainSource{sc});
    return counted(launches);
}

}  // namespace ptss
