// ptss_glare.hip — the kernels behind ptss_glare_build (include/ptss.h): a pyramid of rounded integer averages of what a
// film's integer means hold above a threshold (csrc/ptglare.h has the arithmetic; its host build is the specification). The resolves that
// add it in front of the tone map, ptss_resolve_linear_glare and ptss_resolve_splat_glare, are instantiations of ptss_resolve.hip's kernel.
//
//   glareReduceKernel      film -> d_1. One workgroup per kTile x kTile texels of level 1: the thresholded integer means of the (2 kTile + 2)^2
//                          film pixels under them are staged in LDS, each divided once, and every thread sums its sixteen taps from there
//                          (read straight from the film, every pixel would be divided by four texels: twelve 64-bit divisions a texel)
//   glareDownKernel        d_{k-1} -> d_k in global memory, one thread per texel; glareUpKernel: u_k = d_k + up(u_{k+1}) in place
//   glareTailKernel        one workgroup: from the first level T whose successors and itself fit into LDS together, all remaining downs and
//                          all their ups in one launch, barriers between the levels
//
// Everything is sums of integers: which kernel built a level does not show in the bytes. The one-launch-per-level form (no tail) and the
// untiled reduce are compiled in measurement builds only (PTSS_TUNING_KNOBS); DESIGN.md §3.32 has their timings.
#include "ptss_device.h"
#include "ptfilm.h"
#include "ptglare.h"

#ifdef PTSS_TUNING_KNOBS
#include <cstdlib>
#endif

namespace ptss {

using ptlin::u64;

constexpr int kGlareTile = ptglare::kTile;
constexpr int kGlareStage = ptglare::kStage;
constexpr int kGlareBlock = kGlareTile * kGlareTile;   // the reduce, down and up kernels: one thread per texel of a 16 x 16 tile
constexpr int kGlareTailBlock = ptglare::kTailBlock;

__device__ __forceinline__ void storeEntry(ulonglong2* __restrict__ level, size_t e, const u64* v) {
    level[2 * e] = ulonglong2{v[0], v[1]};
    level[2 * e + 1] = ulonglong2{v[2], 0ull};
}

// the source of the pyramid at film pixel (x, y)
template <bool Splat>
__device__ __forceinline__ void sourceAt(const ulonglong2* __restrict__ film, int width, int x, int y, u64 threshold, u64* v) {
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const ulonglong2 rg = film[2 * p], bw = film[2 * p + 1];
    ptglare::sourceOf(rg.x, rg.y, bw.x, Splat ? bw.y : (bw.y & 0xffffffffull), Splat, threshold, v);
}

// Splat: the film is ptss_splat_entry (word 3 the summed weight), else ptss_linear_entry (its low half the samples). Grid: the tiles of
// level 1, w1 x h1 texels
template <bool Splat>
__global__ __launch_bounds__(kGlareBlock) void glareReduceKernel(const ulonglong2* __restrict__ film, int width, int height, int w1, int h1,
                                                                 u64 threshold, ulonglong2* __restrict__ d1) {
    __shared__ u64 sSrc[3][kGlareStage * kGlareStage];   // three planes: a wave's lanes read neighbouring 8-byte words
    const int x0 = 2 * (int)blockIdx.x * kGlareTile - 1, y0 = 2 * (int)blockIdx.y * kGlareTile - 1;   // the film pixel of slot (0, 0)
    for (int slot = (int)threadIdx.x; slot < kGlareStage * kGlareStage; slot += kGlareBlock) {
        const int lx = slot % kGlareStage, ly = slot / kGlareStage;
        u64 v[3];
        sourceAt<Splat>(film, width, ptglare::clampTo(x0 + lx, width - 1), ptglare::clampTo(y0 + ly, height - 1), threshold, v);
        sSrc[0][slot] = v[0], sSrc[1][slot] = v[1], sSrc[2][slot] = v[2];
    }
    __syncthreads();
    const int i = (int)blockIdx.x * kGlareTile + (int)threadIdx.x % kGlareTile, j = (int)blockIdx.y * kGlareTile + (int)threadIdx.x / kGlareTile;
    if (i >= w1 || j >= h1) return;
    u64 d[3];
    // a tap's clamped film pixel (x, y) lies in x0 .. x0 + 33, y0 .. y0 + 33: 2 i - 1 >= x0 and 2 i + 2 <= x0 + 2 kTile + 1, and clamping to the
    // film only moves it towards the tile
    ptglare::downTexel(i, j, width, height, [&](int x, int y, u64* v) {
        const int slot = (y - y0) * kGlareStage + (x - x0);
        v[0] = sSrc[0][slot], v[1] = sSrc[1][slot], v[2] = sSrc[2][slot];
    }, d);
    storeEntry(d1, (size_t)j * (size_t)w1 + (size_t)i, d);
}

#ifdef PTSS_TUNING_KNOBS
// the form to beat: every texel reads its sixteen film pixels itself and divides each of them
template <bool Splat>
__global__ __launch_bounds__(kGlareBlock) void glareReduceUntiledKernel(const ulonglong2* __restrict__ film, int width, int height, int w1, int h1,
                                                                        u64 threshold, ulonglong2* __restrict__ d1) {
    const int i = (int)blockIdx.x * kGlareTile + (int)threadIdx.x % kGlareTile, j = (int)blockIdx.y * kGlareTile + (int)threadIdx.x / kGlareTile;
    if (i >= w1 || j >= h1) return;
    u64 d[3];
    ptglare::downTexel(i, j, width, height, [&](int x, int y, u64* v) { sourceAt<Splat>(film, width, x, y, threshold, v); }, d);
    storeEntry(d1, (size_t)j * (size_t)w1 + (size_t)i, d);
}
#endif

// src: sw x sh texels; dst: w x h = their halves, rounded up. Grid: the 16 x 16 tiles of dst
__global__ __launch_bounds__(kGlareBlock) void glareDownKernel(const ulonglong2* __restrict__ src, int sw, int sh, ulonglong2* __restrict__ dst, int w,
                                                               int h) {
    const int i = (int)blockIdx.x * kGlareTile + (int)threadIdx.x % kGlareTile, j = (int)blockIdx.y * kGlareTile + (int)threadIdx.x / kGlareTile;
    if (i >= w || j >= h) return;
    u64 d[3];
    ptglare::downTexel(i, j, sw, sh, [&](int x, int y, u64* v) { loadEntry(src, (size_t)y * (size_t)sw + (size_t)x, v); }, d);
    storeEntry(dst, (size_t)j * (size_t)w + (size_t)i, d);
}

// dst: w x h texels holding d_k, u_k afterwards; src: u_{k+1}, cw x ch texels. Grid: the 16 x 16 tiles of dst
__global__ __launch_bounds__(kGlareBlock) void glareUpKernel(const ulonglong2* __restrict__ src, int cw, int ch, ulonglong2* __restrict__ dst, int w,
                                                             int h) {
    const int x = (int)blockIdx.x * kGlareTile + (int)threadIdx.x % kGlareTile, y = (int)blockIdx.y * kGlareTile + (int)threadIdx.x / kGlareTile;
    if (x >= w || y >= h) return;
    u64 u[3], d[3];
    ptglare::upTexel(x, y, cw, ch, [&](int i, int j, u64* v) { loadEntry(src, (size_t)j * (size_t)cw + (size_t)i, v); }, u);
    const size_t e = (size_t)y * (size_t)w + (size_t)x;
    loadEntry(dst, e, d);
    for (int c = 0; c < 3; ++c) d[c] += u[c];
    storeEntry(dst, e, d);
}

// The levels first .. last (1-based) of a pyramid held in LDS together: level k at words 3 * held[k - first] .. of the dynamic LDS, its
// texels in rows, three words each
struct GlareTail {
    int first, last;
    int width[ptglare::kMaxLevels], height[ptglare::kMaxLevels];   // [k - first]
    uint32_t held[ptglare::kMaxLevels];                            // texels of the levels in front of level k, from level `first` on
    unsigned long long entry[ptglare::kMaxLevels];                 // the level's first entry of the pyramid
};

// One workgroup. d_first is in global memory; the downs first + 1 .. last and the ups last - 1 .. first run in LDS, then u_first .. u_last
// are written
__global__ __launch_bounds__(kGlareTailBlock) void glareTailKernel(ulonglong2* __restrict__ pyramid, GlareTail tail) {
    extern __shared__ u64 sTail[];
    const int n = tail.last - tail.first + 1;
    {
        const ulonglong2* level = pyramid + 2 * tail.entry[0];
        const int texels = tail.width[0] * tail.height[0];
        for (int e = (int)threadIdx.x; e < texels; e += kGlareTailBlock) loadEntry(level, (size_t)e, sTail + 3 * e);
    }
    __syncthreads();
    for (int l = 1; l < n; ++l) {   // (uniform: every thread meets every barrier)
        const int w = tail.width[l], h = tail.height[l], sw = tail.width[l - 1], sh = tail.height[l - 1];
        const u64* src = sTail + 3 * tail.held[l - 1];
        u64* dst = sTail + 3 * tail.held[l];
        for (int e = (int)threadIdx.x; e < w * h; e += kGlareTailBlock) {
            u64 d[3];
            ptglare::downTexel(e % w, e / w, sw, sh, [&](int x, int y, u64* v) {
                const u64* t = src + 3 * (y * sw + x);
                v[0] = t[0], v[1] = t[1], v[2] = t[2];
            }, d);
            dst[3 * e] = d[0], dst[3 * e + 1] = d[1], dst[3 * e + 2] = d[2];
        }
        __syncthreads();
    }
    for (int l = n - 2; l >= 0; --l) {
        const int w = tail.width[l], h = tail.height[l], cw = tail.width[l + 1], ch = tail.height[l + 1];
        const u64* src = sTail + 3 * tail.held[l + 1];
        u64* dst = sTail + 3 * tail.held[l];
        for (int e = (int)threadIdx.x; e < w * h; e += kGlareTailBlock) {
            u64 u[3];
            ptglare::upTexel(e % w, e / w, cw, ch, [&](int i, int j, u64* v) {
                const u64* t = src + 3 * (j * cw + i);
                v[0] = t[0], v[1] = t[1], v[2] = t[2];
            }, u);
            dst[3 * e] += u[0], dst[3 * e + 1] += u[1], dst[3 * e + 2] += u[2];
        }
        __syncthreads();
    }
    for (int l = 0; l < n; ++l) {
        ulonglong2* level = pyramid + 2 * tail.entry[l];
        const u64* src = sTail + 3 * tail.held[l];
        const int texels = tail.width[l] * tail.height[l];
        for (int e = (int)threadIdx.x; e < texels; e += kGlareTailBlock) storeEntry(level, (size_t)e, src + 3 * e);
    }
}

static dim3 glareTiles(int w, int h) { return dim3((unsigned)((w + kGlareTile - 1) / kGlareTile), (unsigned)((h + kGlareTile - 1) / kGlareTile)); }

hipError_t launchGlareBuild(hipStream_t st, const void* film, bool splat, int width, int height, const ptss_linear_params& params,
                            const ptss_glare_params& glare, void* pyramid, unsigned long long* launches) {
    const ptglare::Rule R = ptglare::ruleOf(glare, params);
    const int L = glare.levels;
    ptss_glare_level lv[ptglare::kMaxLevels];
    ptglare::layoutOf(width, height, L, lv);
    int T = ptglare::tailLevel(lv, L);
    const ulonglong2* f = static_cast<const ulonglong2*>(film);
    ulonglong2* pyr = static_cast<ulonglong2*>(pyramid);
    auto levelAt = [&](int k) { return pyr + 2 * lv[k - 1].first; };
    const dim3 block(kGlareBlock);
    unsigned long long launched = 0;
    hipError_t e = hipSuccess;
    auto after = [&]() {
        e = hipGetLastError();
        if (e == hipSuccess) ++launched;
        return e == hipSuccess;
    };
    bool tiled = true;
#ifdef PTSS_TUNING_KNOBS   // measurement builds only (tools/build_variants.py "knobs"; tools/glare_bench.py); the shipped library reads no environment
    if (const char* v = getenv("PTSS_GLARE_TAIL")) T = atoi(v) != 0 ? T : L;
    if (const char* v = getenv("PTSS_GLARE_UNTILED")) tiled = atoi(v) == 0;
    if (!tiled) {
        if (splat)
            hipLaunchKernelGGL((glareReduceUntiledKernel<true>), glareTiles(lv[0].width, lv[0].height), block, 0, st, f, width, height, lv[0].width,
                               lv[0].height, R.threshold, levelAt(1));
        else
            hipLaunchKernelGGL((glareReduceUntiledKernel<false>), glareTiles(lv[0].width, lv[0].height), block, 0, st, f, width, height, lv[0].width,
                               lv[0].height, R.threshold, levelAt(1));
    }
#endif
    if (tiled) {
        if (splat)
            hipLaunchKernelGGL((glareReduceKernel<true>), glareTiles(lv[0].width, lv[0].height), block, 0, st, f, width, height, lv[0].width, lv[0].height,
                               R.threshold, levelAt(1));
        else
            hipLaunchKernelGGL((glareReduceKernel<false>), glareTiles(lv[0].width, lv[0].height), block, 0, st, f, width, height, lv[0].width, lv[0].height,
                               R.threshold, levelAt(1));
    }
    bool ok = after();
    for (int k = 2; ok && k <= T; ++k) {
        hipLaunchKernelGGL(glareDownKernel, glareTiles(lv[k - 1].width, lv[k - 1].height), block, 0, st, levelAt(k - 1), lv[k - 2].width,
                           lv[k - 2].height, levelAt(k), lv[k - 1].width, lv[k - 1].height);
        ok = after();
    }
    if (ok && T < L) {
        GlareTail tail;
        tail.first = T;
        tail.last = L;
        uint32_t held = 0u;
        for (int k = T; k <= L; ++k) {
            tail.width[k - T] = lv[k - 1].width;
            tail.height[k - T] = lv[k - 1].height;
            tail.held[k - T] = held;
            tail.entry[k - T] = lv[k - 1].first;
            held += (uint32_t)(lv[k - 1].width * lv[k - 1].height);
        }
        for (int l = L - T + 1; l < ptglare::kMaxLevels; ++l) tail.width[l] = tail.height[l] = 0, tail.held[l] = 0u, tail.entry[l] = 0ull;
        hipLaunchKernelGGL(glareTailKernel, dim3(1), dim3(kGlareTailBlock), (size_t)held * 3u * sizeof(u64), st, pyr, tail);   // held <= kTailEntries
        ok = after();
    }
    for (int k = T - 1; ok && k >= 1; --k) {
        hipLaunchKernelGGL(glareUpKernel, glareTiles(lv[k - 1].width, lv[k - 1].height), block, 0, st, levelAt(k + 1), lv[k].width, lv[k].height,
                           levelAt(k), lv[k - 1].width, lv[k - 1].height);
        ok = after();
    }
    launches[1] += launched;
    if (ok) ++launches[0];
    return e;
}

}  // namespace ptss
