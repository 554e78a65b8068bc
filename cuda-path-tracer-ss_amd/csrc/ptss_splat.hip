// ptss_splat.hip — the kernels behind ptss_splat_paths and ptss_splat_paths_homed (include/ptss.h): a linear film whose
// samples are spread over the pixels around their position by a box, a tent or a Gaussian with integer weights (csrc/ptsplat.h has the
// arithmetic; its host build is the specification). ptss_resolve_splat is an instantiation of ptss_resolve.hip's kernel. Every
// contribution is an integer, so the two forms below leave the same bytes:
//
//   splatScatterKernel   any positions in any order: one lane per sample walks its taps and issues four 64-bit integer atomics per tap
//   splatHomedKernel     sample i sits in the pixel firstPixel + i: one thread per OUTPUT pixel gathers from the homes around it, staged in
//                        LDS once per 16 x 16 tile, and does one plain read-modify-write of its entry. No atomics
#include "ptss_device.h"
#include "ptfilm.h"
#include "ptsplat.h"

namespace ptss {

using ptlin::u64;

constexpr int kSplatBlock = 256;
constexpr int kSplatTile = 16;                            // a workgroup's pixels: 16 x 16
constexpr int kSplatMaxHalo = 2;                          // K = floor(R + 0.5) <= 2
constexpr int kSplatMaxSide = kSplatTile + 2 * kSplatMaxHalo;
constexpr int kSplatMaxSlots = kSplatMaxSide * kSplatMaxSide;
constexpr int kSplatMaxTaps = 5;                          // 2 * reach + 1 candidate columns (rows), at most four of them with weight

// counters[0]: samples dropped, counters[1]: samples with a clamped channel; one atomic per wave each
__global__ __launch_bounds__(kSplatBlock) void splatScatterKernel(const float4* __restrict__ results, const float2* __restrict__ positions, uint32_t n,
                                                                   u64* __restrict__ film, int width, int height, ptspl::Filter F, ptlin::Scale sc,
                                                                   unsigned long long* __restrict__ counters) {
    const uint32_t i = blockIdx.x * kSplatBlock + threadIdx.x;
    const bool inBatch = i < n;
    float2 pos = float2{0.f, 0.f};
    if (inBatch) pos = positions[i];
    const bool dropped = inBatch && (ptspl::outside(pos.x, F.radius, width) || ptspl::outside(pos.y, F.radius, height));
    countDropped(dropped, counters);
    const bool ok = inBatch && !dropped;
    u64 q[3] = {0ull, 0ull, 0ull};
    uint32_t flag = 0u;
    if (ok) {
        const float4 r = results[i];
        flag = ptlin::sampleToFixed(r.x, r.y, r.z, sc, q);
    }
    countDropped(ok && flag != 0u, counters + 1);
    if (!ok) return;
    const int taps = 2 * F.reach + 1;
    const int x0 = ptspl::firstTap(F, pos.x), y0 = ptspl::firstTap(F, pos.y);
    uint32_t wx[kSplatMaxTaps];
#pragma unroll
    for (int a = 0; a < kSplatMaxTaps; ++a) {
        const int x = x0 + a;
        wx[a] = (a < taps && x >= 0 && x < width) ? ptspl::axisWeight(F, pos.x, x) : 0u;   // taps outside the film add nothing
    }
    for (int b = 0; b < taps; ++b) {
        const int y = y0 + b;
        if (y < 0 || y >= height) continue;
        const uint32_t wy = ptspl::axisWeight(F, pos.y, y);
        if (wy == 0u) continue;
        u64* row = film + 4 * ((size_t)y * (size_t)width);
#pragma unroll
        for (int a = 0; a < kSplatMaxTaps; ++a) {
            const uint32_t W = ptspl::tapWeight(wx[a], wy);
            if (W == 0u) continue;   // (wx[a] = 0 for a column outside the film: x0 + a is inside wherever W > 0)
            u64* e = row + 4 * (size_t)(x0 + a);
            atomicAdd(e + 0, ptspl::contribution(q[0], W));
            atomicAdd(e + 1, ptspl::contribution(q[1], W));
            atomicAdd(e + 2, ptspl::contribution(q[2], W));
            atomicAdd(e + 3, (u64)W);
        }
    }
}

// The grid: ceil(width / 16) x ceil((rowHi - rowLo + 1) / 16) tiles over the batch's rows dilated by K = F.halo and clipped to the film
// (rowLo .. rowHi), at full width, so every pixel a sample of the batch can reach has exactly one thread, and no other pixel has one.
// Staging: the homes of the tile and K more on every side, (16 + 2K)^2 <= 400 slots, each its sample's position and three fixed-point
// channels — toFixed runs once per staged sample. A home outside the film or the batch, and a stray, is staged with a NaN position and
// gives nothing. The four staged words live in four arrays of 8-byte elements, not in one 32-byte row: 32 neighbouring lanes then read 32
// neighbouring 8-byte elements, one pass over the 64 banks (a 32-byte stride would put lanes l and l + 8 on one bank, four ways).
// A sample is counted (stray, clamped) by the one tile whose own 16 x 16 pixels hold its home.
__global__ __launch_bounds__(kSplatBlock) void splatHomedKernel(const float4* __restrict__ results, const float2* __restrict__ positions,
                                                                 uint32_t firstPixel, uint32_t n, ulonglong2* __restrict__ film, int width, int height,
                                                                 int rowLo, int rowHi, ptspl::Filter F, ptlin::Scale sc,
                                                                 unsigned long long* __restrict__ counters) {
    __shared__ float2 sPos[kSplatMaxSlots];
    __shared__ u64 sR[kSplatMaxSlots], sG[kSplatMaxSlots], sB[kSplatMaxSlots];
    const int K = F.halo;
    const int side = kSplatTile + 2 * K;
    const int slots = side * side;
    const int tileX = (int)blockIdx.x * kSplatTile, tileY = rowLo + (int)blockIdx.y * kSplatTile;
    for (int base = 0; base < slots; base += kSplatBlock) {   // (every lane takes every trip: the counts below are wave-wide)
        const int s = base + (int)threadIdx.x;
        const bool valid = s < slots;
        const int sy = s / side, sx = s - sy * side;
        const int hx = tileX - K + sx, hy = tileY - K + sy;
        const bool inFilm = valid && hx >= 0 && hx < width && hy >= 0 && hy < height;
        const long long k = (long long)hy * width + hx - (long long)firstPixel;   // the home's sample
        const bool inBatch = inFilm && k >= 0 && k < (long long)n;
        float2 pos = float2{ptm::qnan(), ptm::qnan()};
        u64 q[3] = {0ull, 0ull, 0ull};
        uint32_t flag = 0u;
        bool isStray = false;
        if (inBatch) {
            const float2 at = positions[k];
            isStray = ptspl::stray(at.x, at.y, hx, hy);
            if (!isStray) {
                const float4 r = results[k];
                flag = ptlin::sampleToFixed(r.x, r.y, r.z, sc, q);
                pos = at;
            }
        }
        const bool owned = inBatch && sx >= K && sx < K + kSplatTile && sy >= K && sy < K + kSplatTile;
        countDropped(owned && isStray, counters);
        countDropped(owned && flag != 0u, counters + 1);
        if (valid) {
            sPos[s] = pos;
            sR[s] = q[0];
            sG[s] = q[1];
            sB[s] = q[2];
        }
    }
    __syncthreads();
    const int ty = (int)threadIdx.x / kSplatTile, tx = (int)threadIdx.x - ty * kSplatTile;
    const int px = tileX + tx, py = tileY + ty;
    if (px >= width || py > rowHi) return;   // (rowHi < height)
    u64 sum[4] = {0ull, 0ull, 0ull, 0ull};
    for (int dy = 0; dy <= 2 * K; ++dy) {
        const int rowSlot = (ty + dy) * side + tx;
        for (int dx = 0; dx <= 2 * K; ++dx) {
            const int s = rowSlot + dx;
            const float2 at = sPos[s];
            if (!(at.x == at.x)) continue;   // no sample from this home
            const uint32_t W = ptspl::tapWeight(ptspl::axisWeight(F, at.x, px), ptspl::axisWeight(F, at.y, py));
            if (W == 0u) continue;
            sum[0] += ptspl::contribution(sR[s], W);
            sum[1] += ptspl::contribution(sG[s], W);
            sum[2] += ptspl::contribution(sB[s], W);
            sum[3] += (u64)W;
        }
    }
    if ((sum[0] | sum[1] | sum[2] | sum[3]) == 0ull) return;
    ulonglong2* e = film + 2 * ((size_t)py * (size_t)width + (size_t)px);
    ulonglong2 rg = e[0], bw = e[1];
    rg.x += sum[0];
    rg.y += sum[1];
    bw.x += sum[2];
    bw.y += sum[3];
    e[0] = rg;
    e[1] = bw;
}

hipError_t launchSplatScatter(hipStream_t st, const void* results, const void* positions, uint32_t n, void* film, int width, int height,
                              const ptss_splat_filter& filter, const ptss_linear_params& params, unsigned long long* counters,
                              unsigned long long* launches) {
    hipLaunchKernelGGL(splatScatterKernel, dim3(filmBlocksFor(n, kSplatBlock)), dim3(kSplatBlock), 0, st, static_cast<const float4*>(results),
                       static_cast<const float2*>(positions), n, static_cast<u64*>(film), width, height, ptspl::filterOf(filter),
                       ptlin::scaleOf(params), counters);
    return counted(launches);
}

hipError_t launchSplatHomed(hipStream_t st, const void* results, const void* positions, uint32_t firstPixel, uint32_t n, void* film, int width,
                            int height, const ptss_splat_filter& filter, const ptss_linear_params& params, unsigned long long* counters,
                            unsigned long long* launches) {
    const ptspl::Filter F = ptspl::filterOf(filter);
    const int r0 = (int)(firstPixel / (uint32_t)width), r1 = (int)((firstPixel + n - 1u) / (uint32_t)width);   // n > 0
    const int rowLo = r0 - F.halo > 0 ? r0 - F.halo : 0, rowHi = r1 + F.halo < height - 1 ? r1 + F.halo : height - 1;
    const dim3 grid((unsigned)((width + kSplatTile - 1) / kSplatTile), (unsigned)((rowHi - rowLo + kSplatTile) / kSplatTile));
    hipLaunchKernelGGL(splatHomedKernel, grid, dim3(kSplatBlock), 0, st, static_cast<const float4*>(results), static_cast<const float2*>(positions),
                       firstPixel, n, static_cast<ulonglong2*>(film), width, height, rowLo, rowHi, F, ptlin::scaleOf(params), counters);
    return counted(launches);
}

}  // namespace ptss
