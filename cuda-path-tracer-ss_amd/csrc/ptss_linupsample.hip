// ptss_linupsample.hip — the kernels behind ptss_upsample_linear (include/ptss.h): a linear or a filtered linear film
// of W x H rebuilt as a linear film of f W x f H in linear light, guided by the features of both sizes. The arithmetic is
// csrc/ptlinup.h, shared with the host probe (ptss_probe_upsample_linear, the specification); this file only moves the data.
//
// One thread per HI pixel, workgroups of 32 x 8 hi pixels laid out as one row of workgroups (a film 2^22 pixels high has more tile rows
// than a grid has in y, and ptss_upsample's 524,280-row limit comes from there); the factor is a template argument, so the divisions
// and remainders of the tap geometry are multiplications and shifts. Per hi pixel both 16-byte rows of its own feature, the depth words
// of its four hi-res neighbours, and one 32-byte film row written. The two forms of linUpsampleKernel differ in how the four taps arrive:
//
//   <kStaged = false>         each tap's 32-byte film entry, 16-byte geometry row and material word from global memory, at clamped
//                             coordinates and all issued before the first test (ptlup::upsamplePixel arranges that); the 64-bit
//                             divisions of the means — three per entry, seven on a filtered film, and gfx950 has no instruction for
//                             them — run once per COUNTED tap: up to twelve (28) per hi pixel
//   <kStaged = true>          the lo pixels a tile's taps can reach — the 32 / f x 8 / f under the tile and a ring of one around them:
//                             33 x 9, 18 x 6, 13 x 5, 10 x 4 slots for f = 1..4 — are read and DIVIDED once, by one thread each, and
//                             staged in LDS as {m_r, m_g} {m_b, K} (two 16-byte rows), the geometry row and the material word: 52 B a
//                             slot, 15.1, 5.5, 3.3 and 2.0 KiB a workgroup, which never limits the occupancy (160 KiB a compute unit).
//                             A slot outside the film holds the pixel its coordinates clamp to (with the wrap: wrap to), exactly what
//                             the global form reads there, so a tile that is all halo, the frame's border and the seam need no case
//                             of their own. Lanes of a wave read neighbouring or equal slots: ds_read_b128 serves both without bank
//                             conflicts, so the rows are not padded
//
// Both call ptlup::upsamplePixel and give the same bytes; which factor runs which form by default is kLinUpsampleStagedAt below. The counters of
// ptss_upsample_linear_info: a wave's ballots are counted on the scalar unit and lane 0 of each wave adds the non-zero ones to the
// caller's with one 64-bit vector atomic each — one wave reduction, at most three atomics a wave, none when dev_info is NULL; integer
// adds, the same bytes for every launch shape. No workgroup waits for another; no bit of ptss_launched_kernels.
#include <hip/hip_runtime.h>

#include "ptlinup.h"
#include "ptss_device.h"

namespace ptss {

using ptlin::u64;

constexpr int kLinUpsampleTileX = 32, kLinUpsampleTileY = 8;
constexpr int kLinUpsampleBlock = kLinUpsampleTileX * kLinUpsampleTileY;

// the slots of a staged tile along an axis of `tile` hi pixels, the lower tap of the first pixel to the upper tap of the last: the lower
// tap of hi pixel X is floor((2 X + 1 - f) / 2 f), which moves by at most ceil((tile - 1) / f) across the tile
constexpr int linUpsampleSlots(int tile, int f) { return (tile - 1 + f - 1) / f + 2; }

// The form per factor f = 1..4 the library ships: true = staged. Measured to 1080p and 2160p (tools/upsample_linear_bench.py; DESIGN.md
// §3.36), the staged form against the global one, five interleaved pairs each: at f = 2, 3, 4 staged is faster in every pair on both
// films (to 1080p the filtered film 0.055 to 0.057 against 0.112 to 0.116 ms, the linear film 0.048 to 0.051 against 0.053 to 0.057 ms).
// At f = 1 the evidence is mixed — linear 0.0561 against 0.0587 ms, filtered 0.0603 against 0.0561 ms, slower in every pair: one tap
// counts per hi pixel there, so the global form divides once per pixel too, and 297 slots are divided for 256 pixels — and the form
// without LDS ships. (Both forms stay compiled at every factor for the tests and the measurement.)
constexpr bool kLinUpsampleStagedAt[ptlup::kMaxFactor] = {false, true, true, true};

__device__ __forceinline__ void linUpsampleCount(int status, unsigned long long* __restrict__ info) {
    const uint32_t filtered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(status == ptlup::kFiltered));
    const uint32_t fallback = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(status == ptlup::kFallback));
    const uint32_t empty = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(status == ptlup::kEmpty));
    if ((threadIdx.x & 63u) == 0u) {
        if (filtered) atomicAdd(&info[0], (unsigned long long)filtered);
        if (fallback) atomicAdd(&info[1], (unsigned long long)fallback);
        if (empty) atomicAdd(&info[2], (unsigned long long)empty);
    }
}

template <int kFactor, bool kSplat, bool kStaged>
__global__ __launch_bounds__(kLinUpsampleBlock) void linUpsampleKernel(const ulonglong2* __restrict__ filmLo, const float4* __restrict__ featuresLo,
                                                                       const float4* __restrict__ featuresHi, ulonglong2* __restrict__ filmHi,
                                                                       unsigned long long* __restrict__ info, int width, int height, int tilesX,
                                                                       ptlup::Rule R) {
    using namespace ptv;
    R.factor = kFactor;   // (the caller's value; as a constant here)
    constexpr int kW = linUpsampleSlots(kLinUpsampleTileX, kFactor), kH = linUpsampleSlots(kLinUpsampleTileY, kFactor);
    constexpr int kSlots = kStaged ? kW * kH : 1;
    __shared__ ulonglong2 sMeansRG[kSlots];
    __shared__ ulonglong2 sMeanBK[kSlots];
    __shared__ float4 sGeometry[kSlots];
    __shared__ int sMaterial[kSlots];
    const int tileX = (int)(blockIdx.x % (unsigned)tilesX), tileY = (int)(blockIdx.x / (unsigned)tilesX);
    const int X0 = tileX * kLinUpsampleTileX, Y0 = tileY * kLinUpsampleTileY;
    const int hiW = width * kFactor, hiH = height * kFactor;   // < 2^31 pixels together: ptss_upsample_linear checks
    // the lo pixel of slot (0, 0): the lower tap of the tile's first pixel; the lower taps do not decrease along an axis
    const int loX0 = ptup::axisOf(X0, kFactor).x0, loY0 = ptup::axisOf(Y0, kFactor).x0;
    if constexpr (kStaged) {
        const bool wrap = R.wrap != 0;
        for (int slot = (int)threadIdx.x; slot < kSlots; slot += kLinUpsampleBlock) {
            const int tx = loX0 + slot % kW;   // >= -1; a slot right of column `width` is never a tap and takes that column's pixel
            const int cx = ptlup::clamped(ptlup::wrapped(tx > width ? width : tx, width, wrap), width);
            const int cy = ptlup::clamped(loY0 + slot / kW, height);
            const size_t q = (size_t)cy * (size_t)width + (size_t)cx;
            const ulonglong2 rg = filmLo[2 * q], bw = filmLo[2 * q + 1];
            const ptlup::Lo lo = ptlup::loOf(rg.x, rg.y, bw.x, bw.y, kSplat);
            sMeansRG[slot] = ulonglong2{lo.m[0], lo.m[1]};
            sMeanBK[slot] = ulonglong2{lo.m[2], lo.K};
            sGeometry[slot] = featuresLo[2 * q];
            sMaterial[slot] = reinterpret_cast<const int*>(featuresLo)[8 * q + 7];
        }
        __syncthreads();
    }
    const int X = X0 + (int)(threadIdx.x % kLinUpsampleTileX), Y = Y0 + (int)(threadIdx.x / kLinUpsampleTileX);
    int status = -1;
    if (X < hiW && Y < hiH) {   // every access below is to hi pixel (X, Y), or at coordinates upsamplePixel has clamped into a frame
        const size_t p = (size_t)Y * (size_t)hiW + (size_t)X;
        const float4 r0 = featuresHi[2 * p];
        const ptdn::Feature fp{v3(r0.x, r0.y, r0.z), r0.w, reinterpret_cast<const int*>(featuresHi)[8 * p + 7]};
        // staged: a tap lies in [x0 of the tile's first pixel, x0 + 1 of its last] along each axis: its slot is inside the rectangle
        auto tapAt = [&](int tx, int ty, int cx, int cy, u64* e) {
            if constexpr (kStaged) {
                const int slot = (ty - loY0) * kW + (tx - loX0);
                const ulonglong2 a = sMeansRG[slot], b = sMeanBK[slot];
                e[0] = a.x, e[1] = a.y, e[2] = b.x, e[3] = b.y;
            } else {
                const size_t q = (size_t)cy * (size_t)width + (size_t)cx;
                const ulonglong2 rg = filmLo[2 * q], bw = filmLo[2 * q + 1];
                e[0] = rg.x, e[1] = rg.y, e[2] = bw.x, e[3] = bw.y;
            }
        };
        auto featureAt = [&](int tx, int ty, int cx, int cy) -> ptdn::Feature {
            if constexpr (kStaged) {
                const int slot = (ty - loY0) * kW + (tx - loX0);
                const float4 g = sGeometry[slot];
                return ptdn::Feature{v3(g.x, g.y, g.z), g.w, sMaterial[slot]};
            } else {
                const size_t q = (size_t)cy * (size_t)width + (size_t)cx;
                const float4 g = featuresLo[2 * q];
                return ptdn::Feature{v3(g.x, g.y, g.z), g.w, reinterpret_cast<const int*>(featuresLo)[8 * q + 7]};
            }
        };
        auto depthAt = [&](int x, int y) -> float { return reinterpret_cast<const float*>(featuresHi)[8 * ((size_t)y * (size_t)hiW + (size_t)x) + 3]; };
        u64 o[4];
        status = ptlup::upsamplePixel<kStaged>(X, Y, width, height, R, kSplat, fp, tapAt, featureAt, depthAt, o);
        filmHi[2 * p] = ulonglong2{o[0], o[1]};
        filmHi[2 * p + 1] = ulonglong2{o[2], o[3]};
    }
    if (info) linUpsampleCount(status, info);   // wave-uniform: a kernel argument
}

using LinUpsampleFn = void (*)(const ulonglong2*, const float4*, const float4*, ulonglong2*, unsigned long long*, int, int, int, ptlup::Rule);

template <int kFactor>
static LinUpsampleFn linUpsampleOf(bool splat, bool staged) {
    return splat ? (staged ? linUpsampleKernel<kFactor, true, true> : linUpsampleKernel<kFactor, true, false>)
                 : (staged ? linUpsampleKernel<kFactor, false, true> : linUpsampleKernel<kFactor, false, false>);
}

hipError_t launchLinearUpsample(hipStream_t st, const void* filmLo, bool splat, int width, int height, const void* featuresLo,
                                const void* featuresHi, const ptss_linear_params& film, const ptss_upsample_linear_params& params, int form,
                                void* filmHi, void* info, unsigned long long* launches) {
    const int f = params.factor;
    if (f < 1 || f > ptlup::kMaxFactor) return hipErrorInvalidValue;
    // form: 0 the measured table, 1 from global memory, 2 staged
    const bool staged = form == 2 || (form == 0 && kLinUpsampleStagedAt[f - 1]);
    const LinUpsampleFn fn = f == 1 ? linUpsampleOf<1>(splat, staged)
                                    : (f == 2 ? linUpsampleOf<2>(splat, staged) : (f == 3 ? linUpsampleOf<3>(splat, staged) : linUpsampleOf<4>(splat, staged)));
    // the tiles of the large film as one row of workgroups; below 2^31 / 256 + 2^22 / 8 + 2^22 / 32
    const int hiW = width * f, hiH = height * f;
    const int tilesX = (hiW + kLinUpsampleTileX - 1) / kLinUpsampleTileX, tilesY = (hiH + kLinUpsampleTileY - 1) / kLinUpsampleTileY;
    const dim3 grid((unsigned)tilesX * (unsigned)tilesY);
    hipLaunchKernelGGL(fn, grid, dim3(kLinUpsampleBlock), 0, st, static_cast<const ulonglong2*>(filmLo), static_cast<const float4*>(featuresLo),
                       static_cast<const float4*>(featuresHi), static_cast<ulonglong2*>(filmHi), static_cast<unsigned long long*>(info), width,
                       height, tilesX, ptlup::ruleOf(params, film));
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++*launches;
    return e;
}

}  // namespace ptss
